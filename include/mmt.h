/* mmt.h — C-ABI of libmmt_hip.so, the MI355X-native (gfx950) training hot path of the
 * multimodal transformer of tsnuk/trade-AId-multimodal-transformer.
 *
 * The reference exposes no C / FFI boundary on this path: its boundary is the
 * Python module API that main.py imports. Each entry point below replaces one piece of that
 * Python surface; the Python host layer (trade-aid-multimodal-transformer_amd/model.py,
 * mmt_optim.py, training_utils.py) binds them through ctypes exactly as INTEGRATION.md shows.
 *
 *   mmt_create / mmt_destroy      <- MultimodalTransformer.__init__ (reference model.py:358-370):
 *                                    dims from config_utils (model.py:25-27), cross flags from
 *                                    all_modality_params[i][8] (model.py:196)
 *   mmt_tensor_count/_info        <- MultimodalTransformer.state_dict() key set and shapes
 *                                    (reference main.py:470, 635) over one flat fp32 buffer
 *   mmt_forward                   <- MultimodalTransformer.forward(idx_list, targets_list)
 *                                    (model.py:380-402): logits per modality + mean CE losses
 *   mmt_backward[_stage]          <- total_loss.backward() of main.py:646-649 (autograd over
 *                                    model.py), gradients into a flat fp32 buffer
 *   mmt_adamw_step                <- torch.optim.AdamW(m.parameters(), lr).step() (main.py:464, 650)
 *   mmt_decode_step               <- one token of MultimodalTransformer.generate (model.py:404-446),
 *                                    with a KV cache instead of the reference's full re-forward
 *   mmt_sample                    <- the sampling line of generate (model.py:425-427: softmax + multinomial),
 *                                    extended by temperature, top-k, top-p, seeded draws and log-probabilities
 *   mmt_sample_multi              <- the same line for several modalities of one step (a joint rollout), one launch
 *   mmt_eval_direction            <- the per-sample loop of calculate_evaluation_metrics
 *                                    (training_utils.py:259-304)
 *   mmt_op_*                      primitive kernels, exported for kernel-level parity tests.
 *
 * Conventions: every pointer is a device pointer unless stated; memory is owned by the caller
 * (PyTorch allocates parameters, gradients, moments, logits and the workspace); the library
 * never frees caller memory. All work is asynchronous on the caller's HIP stream (`stream` is a
 * hipStream_t passed as void*). Every function returns 0 (MMT_OK) or a negative mmt_status;
 * no C++ exception crosses the ABI; mmt_last_error() describes the last failure.
 */
#ifndef MMT_H_
#define MMT_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMT_MAX_MODALITIES 8

enum mmt_status {
  MMT_OK = 0,
  MMT_ERR_INVALID = -1,     /* bad argument / shape */
  MMT_ERR_UNSUPPORTED = -2, /* configuration outside what the kernels implement */
  MMT_ERR_HIP = -3,         /* a HIP runtime call or launch failed */
  MMT_ERR_STATE = -4        /* call order violated (e.g. backward without matching forward) */
};

typedef struct mmt_config {
  int32_t num_modalities;                       /* M, 1..8 */
  int32_t n_embd;                               /* C */
  int32_t n_head;                               /* H, head size C/H in {8,16,24,32,48,64} */
  int32_t n_layer;                              /* L */
  int32_t block_size;                           /* T (max sequence length, positional table rows) */
  int32_t vocab_sizes[MMT_MAX_MODALITIES];      /* V_i >= 1 */
  int32_t cross_attention[MMT_MAX_MODALITIES];  /* all_modality_params[i][8] */
  float dropout;                                /* nn.Dropout p (model.py:57,87,107,134,171) */
  uint64_t seed;                                /* dropout RNG seed */
  int32_t precision;                            /* 0: bf16 MFMA; 1: MX-fp8 forward GEMMs (C4;
                                                   Q/K/V stage 1, FFN, cross-attention query;
                                                   needs n_embd % 32 == 0) */
} mmt_config;

typedef struct mmt_ctx mmt_ctx;

/* lifecycle */
mmt_ctx* mmt_create(const mmt_config* cfg); /* NULL on failure, see mmt_create_error() */
const char* mmt_create_error(void);
void mmt_destroy(mmt_ctx* ctx);
const char* mmt_last_error(const mmt_ctx* ctx);
const char* mmt_version(void);

/* parameter layout: one flat fp32 buffer; each reference state_dict tensor is a contiguous slice */
int64_t mmt_param_count(const mmt_ctx* ctx);        /* elements of the flat buffer */
int64_t mmt_param_active_count(const mmt_ctx* ctx); /* prefix that receives gradients */
int32_t mmt_tensor_count(const mmt_ctx* ctx);
int mmt_tensor_info(const mmt_ctx* ctx, int32_t i, char* name, int32_t name_cap, int64_t* offset, int32_t* ndim,
                    int64_t* shape /* [2] */, int32_t* kind /* 0 weight(N(0,.02)) 1 bias(0) 2 ln weight(1) 3 ln bias(0) */);

/* workspace (saved activations + packed bf16 weights + backward scratch) for a batch size */
int64_t mmt_workspace_bytes(mmt_ctx* ctx, int32_t batch);

/* forward: idx[i], tgt[i] int64 [batch, T] (tgt may be NULL: no loss); logits[i] fp32 [batch, T, V_i];
 * losses fp32 [M] (per modality the mean CE, or the objective of mmt_set_loss; written only when tgt != NULL);
 * training != 0 enables dropout */
int mmt_forward(mmt_ctx* ctx, void* stream, int32_t batch, const int64_t* const* idx, const int64_t* const* tgt,
                const float* params, float* const* logits, float* losses, void* workspace, int32_t training);

/* KV-cache decode step of generate (reference model.py:404-446, which re-runs the whole forward
 * per new token): the forward of ONE new position `pos` (1 <= pos < block_size) of every sequence
 * and modality. idx[i]: int64 [batch] tokens of modality i at position pos; logits[i]: fp32
 * [batch, V_i], the logits at position pos. Keys / values of positions < pos come from the last
 * mmt_forward on this workspace (the prefill: prompt right-padded to block_size) and the decode
 * steps since, which this step extends by position pos. Eval semantics (no dropout); the weights
 * are the ones packed by that prefill forward. MMT_ERR_STATE without a prefill, after a prefill
 * that sampled dropout (training != 0 with dropout > 0: its keys / values are not the eval ones),
 * and at precision fp8 (the prefill's MX-fp8 GEMMs would not match a bf16 decode). */
int mmt_decode_step(mmt_ctx* ctx, void* stream, int32_t batch, int32_t pos, const int64_t* const* idx,
                    const float* params, float* const* logits, void* workspace);

/* Sample fan-out (generate with num_samples = S): S continuations of each of `batch` prompts share ONE prefill
 * and the prompt's keys / values. The decode step runs over batch*samples compact rows, row r = b*samples + s
 * being sample s of prompt b, in a caller-owned fan buffer (the library still never allocates):
 *   mmt_fanout_bytes        its size: the compact [batch*samples, *] scratch of one step plus the tail caches, per
 *                           (layer, modality) the self-attention tail bf16 [batch*samples, max_new, 3C] and per
 *                           (layer, cross modality, KV stream) the cross tail [batch*samples, max_new, 2C], row
 *                           r*max_new + (pos - n0), columns as the forward's Q/K/V and cross K/V rows. -1 for
 *                           batch, samples or max_new < 1, max_new >= block_size, or batch*samples rows beyond
 *                           the launchers' 32-bit row * column range.
 *   mmt_decode_fanout_step  the forward of position `pos` of every row: idx[i] int64 [batch*samples], logits[i]
 *                           fp32 [batch*samples, V_i]. Keys / values of positions < n0 of row r are the workspace
 *                           cache rows of sequence r / samples (what the last mmt_forward at `batch`, and any
 *                           mmt_decode_step since, left there); positions n0..pos come from the fan buffer, which
 *                           this step extends by position pos. The workspace is only read: after any number of
 *                           fan-out steps mmt_decode_step at n0 gives the bits it gave before them.
 * A run starts with pos == n0 (tail row 0) and continues with pos one greater per call, pos < n0 + max_new <=
 * block_size; the engine keeps (n0, samples, next pos). MMT_ERR_STATE for a call out of order, without a prefill,
 * after a prefill that sampled dropout and at precision fp8; MMT_ERR_INVALID for a null pointer, samples / n0 /
 * max_new < 1, n0 + max_new > block_size, pos outside n0..n0+max_new-1, and after a training forward that kept
 * Q/K/V on chip (as mmt_decode_step). Every refusal returns before any launch. A new mmt_forward ends the run. */
int64_t mmt_fanout_bytes(mmt_ctx* ctx, int32_t batch, int32_t samples, int32_t max_new);
int mmt_decode_fanout_step(mmt_ctx* ctx, void* stream, int32_t batch, int32_t samples, int32_t n0, int32_t max_new,
                           int32_t pos, const int64_t* const* idx, const float* params, float* const* logits,
                           const void* workspace, void* fan);

/* Rolling-window step (generate with num_samples and rolling=True, past block_size): the paths of a prompt share
 * the first p rows of their block_size window (the prompt's rows, shifted) and differ only in the last m rows, the
 * tokens generated so far. One step recomputes those m rows of every path through all layers, over batch*samples*m
 * compact rows (row r*m + i: tail position i of path r = b*samples + s, at position p + i), and returns the logits
 * of each path's last row. Cost in rows through the layers: batch*p for the prefix forward plus batch*samples*m,
 * where the tiled re-forward takes batch*samples*block_size.
 *   mmt_rolling_bytes  the size of the caller-owned roll buffer for tails of up to max_tail rows: the compact
 *                      scratch of one step, batch*samples*max_tail rows. The paths' own keys / values are that
 *                      scratch's K|Q|V and cross-K/V rows of the layer in flight and the residual rows rotate over
 *                      two layer slots, so the size does not depend on n_layer. -1 for batch, samples or max_tail
 *                      < 1, max_tail >= block_size, or rows beyond the launchers' 32-bit row * column range.
 *   mmt_rolling_step   idx[i] points at the first tail token of row 0 of modality i inside an int64 [rows, idx_ld]
 *                      buffer: tail token i of path r is idx[i][r*idx_ld + i] (idx_ld >= m; no token is copied).
 *                      logits[i] is fp32 [batch*samples, V_i]. Keys / values of positions < p of path r are the
 *                      workspace cache rows of sequence r / samples: the last mmt_forward on `workspace` must have
 *                      been over `batch` sequences whose first p positions are the shared prefix (the engine
 *                      checks the batch, not the length). The workspace is only read, and the roll buffer holds
 *                      nothing between calls: any (p, m) with p >= 1, m >= 1, p + m <= block_size and a buffer of
 *                      mmt_rolling_bytes(batch, samples, max_tail >= m) is valid after such a forward, in any order,
 *                      and the same call twice gives the same bits. bf16, eval semantics.
 * MMT_ERR_STATE without such a forward (another batch included), after a forward that sampled dropout and at
 * precision fp8; MMT_ERR_INVALID for a null pointer, samples / p / m < 1, p + m > block_size, idx_ld < m, rows
 * beyond the launchers' range, and after a training forward that kept Q/K/V on chip. Every refusal returns before
 * any launch and leaves logits alone. The launches carry roll_* labels (mmt_probe_set). */
int64_t mmt_rolling_bytes(mmt_ctx* ctx, int32_t batch, int32_t samples, int32_t max_tail);
int mmt_rolling_step(mmt_ctx* ctx, void* stream, int32_t batch, int32_t samples, int32_t p, int32_t m,
                     const int64_t* const* idx, int64_t idx_ld, const float* params, float* const* logits,
                     const void* workspace, void* roll);

/* Device-side sampling of generate (reference model.py:425-427: softmax of the last logits, torch.multinomial,
 * nothing else): one token per row from fp32 logits with temperature, top-k and top-p, a draw keyed by
 * (seed, row, position), and the log-probability of the token, in ONE launch for all rows (one 256-thread
 * workgroup per row). Needs no context: any fp32 buffer. Row b is read at logits + b * row_stride (elements,
 * row_stride >= V), so the last position of a prefill's [B, T, V] tensor is read in place (pointer offset
 * (n - 1) * V, stride T * V) as well as a decode step's [B, V]. The rule, per row:
 *   1. z_i = logits_i * (1 / temperature): 1 / temperature is one fp32 division on the host, the product one
 *      fp32 multiply; a NaN z counts as -inf. m = max z.
 *   2. top-k (0 < top_k < V; 0 = off): t_k = the top_k-th largest z, duplicates counted; kept = { i : z_i >= t_k }
 *      (ties at the threshold are all kept; comparisons only, exact).
 *   3. e_i = exp(z_i - m) on the kept set (1 where z_i == m), 0 elsewhere; S = sum e_i.
 *   4. top-p (top_p < 1; >= 1 = off): over the distinct kept values of z in descending order, t_p = the first at
 *      which the mass of { z_i >= t_p } reaches top_p * S; kept = { z_i >= t_p } (ties kept), S recomputed.
 *      top_p <= 0 keeps the maximal group only.
 *   5. key = mmt_hash(lo32(seed), hi32(seed), 0x53414D50); h = mmt_hash(key, row0 + b, pos);
 *      u = ((h >> 8) + 0.5) * 2^-24, with mmt_hash the dropout masks' counter hash
 *      (h = a * 0x9E3779B1 ^ (b + 0x7F4A7C15) * 0x85EBCA77 ^ (c + 0x165667B1) * 0xC2B2AE3D; h ^= h >> 16;
 *      h *= 0x7FEB352D; h ^= h >> 15; h *= 0x846CA68B; h ^= h >> 16, all modulo 2^32).
 *   6. the token is the first index in vocabulary order whose inclusive prefix sum of e reaches u * S; it always
 *      has e > 0.
 *   7. the log-probability is log(e_tok / S), fp32, under the distribution actually sampled from (computed as
 *      (z_tok - m) - log S).
 * temperature == 0 is greedy: the lowest index among the maxima of the raw logits (NaN as -inf), top_k and top_p
 * ignored, the log-probability the raw log-softmax at that token. A row with no finite logit (every entry -inf or
 * NaN) gives token 0 and log-probability NaN; no kernel traps.
 * Outputs: the token as int64 at tok + b * tok_stride (column n of a [B, cap] sequence buffer is written in
 * place); if tok_compact != NULL also at tok_compact[b] (what mmt_decode_step takes as idx[g] of the next
 * position); if logprob != NULL the log-probability at logprob + b * lp_stride.
 * The weights e are fp32 (expf), their sums fp64 over a fixed assignment and a fixed tree (no float atomics): a
 * launch is bit-identical run to run,
 * and row b of a launch equals the same row launched alone with row0 + b as its row0. Rows up to V = 8192 stay in
 * LDS; larger ones (to V = 2^20, above that MMT_ERR_UNSUPPORTED) are re-read from memory.
 * MMT_ERR_INVALID before any launch for: batch < 0, V < 1, row_stride < V, temperature negative or NaN,
 * top_k < 0, top_p NaN, a null logits / tok with batch > 0. batch == 0 launches nothing. */
int mmt_sample(void* stream, int32_t batch, int32_t V, const float* logits, int64_t row_stride, float temperature,
               int32_t top_k, float top_p, uint64_t seed, uint32_t row0, uint32_t pos, int64_t* tok,
               int64_t tok_stride, int64_t* tok_compact /* nullable */, float* logprob /* nullable */,
               int64_t lp_stride);

/* Several heads of one step in ONE launch (a joint rollout of generate samples every generated modality per token;
 * at C1 a decode token is launch-bound, so G launches of mmt_sample are G - 1 too many): `count` independent
 * problems over the same `batch` rows, `row0` and `pos`, grid (rows, problems). Every other argument of mmt_sample
 * is a HOST array of `count` entries, read during the call (as the pointer arrays of mmt_forward): V, logits,
 * row_stride, temperature, top_k, top_p, seed, tok, tok_stride, tok_compact, logprob, lp_stride. The arrays
 * tok_compact and logprob may be NULL (no problem has that output), and so may any of their entries; lp_stride is
 * read only where logprob is given.
 * The contract: problem p gives bit for bit what mmt_sample gives when called alone with problem p's arguments
 * (tokens, compact tokens, log-probabilities): both kernels are one device function, and a row's result depends
 * on nothing else in the launch. In a joint rollout problem p carries its modality's own seed (the keying rule:
 * INTEGRATION.md, mmt_sample.modality_seed), so draws of different modalities are independent.
 * Launches: when every V is at most 8192 (the LDS rows) and count <= 8, one. Problems with V > 8192 run the
 * re-read variant in a SECOND launch of the same shape (no runtime branch in the kernel: the LDS rows keep their
 * code and the re-read rows do not reserve 32 KiB of LDS); more than 8 problems of either kind go in chunks of 8.
 * All problems are validated before any launch, each by mmt_sample's own rules, the first failing problem giving
 * the status (MMT_ERR_INVALID, or MMT_ERR_UNSUPPORTED for V > 2^20): then nothing is written. Also
 * MMT_ERR_INVALID: count < 0, batch < 0, with count > 0 a null V / logits / row_stride / temperature / top_k /
 * top_p / seed / tok / tok_stride array, or logprob without lp_stride. count == 0 or batch == 0 launches nothing
 * (batch == 0 after the validation, as mmt_sample). No knobs, no atomics, the summation trees of mmt_sample. */
int mmt_sample_multi(void* stream, int32_t count, int32_t batch, const int32_t* V, const float* const* logits,
                     const int64_t* row_stride, const float* temperature, const int32_t* top_k, const float* top_p,
                     const uint64_t* seed, uint32_t row0, uint32_t pos, int64_t* const* tok,
                     const int64_t* tok_stride, int64_t* const* tok_compact /* nullable, entries nullable */,
                     float* const* logprob /* nullable, entries nullable */, const int64_t* lp_stride);

/* Evidence of conditioned rollouts. generate(..., given={i: tokens}) forces modality i through the caller's series;
 * the heads are conditionally independent given the history, so the probability of the forced token under its own
 * head is the path's importance weight. The three entries below score the forced tokens, turn weighted paths into
 * posterior paths (a particle filter over the S paths of a prompt) and move the fan-out tails to their ancestors.
 *
 * mmt_score_multi: `count` problems over the same `batch` rows, grid (rows, problems), the shape and the host
 * arrays of mmt_sample_multi. Problem p reads row b of its fp32 logits at logits[p] + b * row_stride[p] (a
 * [B, T, V] tensor is read in place) and the token tok[p][b * tok_stride[p]] (int64), and writes the fp32
 * log-probability at logprob[p] + b * lp_stride[p].
 * The rule: the score of token t is the log-probability mmt_sample reports when it draws t at temperature 1,
 * top_k 0, top_p 1: steps 1, 3 and 7 above (z = logit, NaN as -inf; e_i = exp(z_i - m) in fp32, 1 at the maximum;
 * S their fp64 sum over the sampler's tree; (z_t - m) - log S rounded to fp32 once), by the sampler's own device
 * code, so the score is bit for bit what the sampler writes for the same row and token. A token whose logit is
 * -inf or NaN scores -inf; a row with no finite logit scores NaN; a token outside 0..V-1 (which the Python layer
 * refuses before any launch) is not read and scores NaN.
 * MMT_ERR_INVALID before any launch, nothing written: count < 0, batch < 0, with count > 0 a null array, and per
 * problem V < 1, row_stride < V or, with batch > 0, a null logits / tok / logprob; MMT_ERR_UNSUPPORTED for
 * V > 2^20. All problems are checked before any launch. Launches as mmt_sample_multi: chunks of 8 problems, rows
 * with V > 8192 in the re-read variant. mmt_sample and mmt_sample_multi keep their launch shapes and bits. */
int mmt_score_multi(void* stream, int32_t count, int32_t batch, const int32_t* V, const float* const* logits,
                    const int64_t* row_stride, const int64_t* const* tok, const int64_t* tok_stride,
                    float* const* logprob, const int64_t* lp_stride);

/* mmt_resample: one workgroup per prompt, no context. Row r = b * samples + s is path s of prompt b. Inputs:
 * `count` <= 8 log-probability matrices (the given modalities', fp32, logprob[i] + r * lp_stride[i] + j; HOST
 * arrays of pointers and strides), the column range [j0, j1), logw fp64 [batch * samples] (the log-weight carried
 * since the last resampling; the caller zeroes it at the start), log_evidence fp64 [batch] (accumulated; zeroed by
 * the caller), ess_threshold, seed, pos. Outputs: ancestors int32 [batch * samples] as GLOBAL row indices,
 * resampled int32 [batch]. The rule, per prompt b, with S = samples:
 *   1. a_s = logw[r] + sum over j = j0..j1-1, then over the given matrices in the caller's order (ascending
 *      modality), of (double) lp_i[r, j]: a serial fp64 sum in that order; a NaN term (and a NaN logw or sum)
 *      counts as -inf. mx = max a_s. If mx == -inf (no live path): logw[r] = a_s, ancestors are the identity,
 *      resampled[b] = 0, nothing else is written.
 *   2. d_s = (float)(a_s - mx); e_s = 1 where d_s == 0, else expf(d_s), fp32. W = sum e_s and Q = sum e_s^2 in fp64
 *      over a fixed assignment and tree, the sampler's: thread t of 256 owns the c = ceil(S / 256) | 1 consecutive
 *      elements from t c, serial sum, shift scan over the lanes, wave totals added left to right.
 *      ESS = W^2 / Q.
 *   3. if not ESS < ess_threshold * S (fp64): logw[r] = a_s, ancestors are the identity, resampled[b] = 0.
 *   4. else systematic resampling: key = mmt_hash(lo32(seed), hi32(seed), 0x52534D50); h = mmt_hash(key, b, pos);
 *      u = ((h >> 8) + 0.5) * 2^-24. Slot s takes the first row, in row order, with e > 0 whose inclusive prefix
 *      sum of e (the tree's) reaches ((s + u) / S) * W; if rounding leaves none, the last row with e > 0.
 *      ancestors[r] = b * S + that row, logw[r] = 0, log_evidence[b] += mx + log(W / S), resampled[b] = 1.
 * Hence equal weights give the identity, and a dead path (e = 0) is never an ancestor. ess_threshold 0 never
 * resamples: the call only folds the columns into logw. A NEGATIVE ess_threshold is the closing fold of a run: no
 * resampling (steps 1 and 3), and log_evidence[b] += mx + log(W / S) (-inf when no path is live), so log_evidence
 * ends as the estimate of log p(given series | history) and logw as the weights of the returned paths.
 * No float atomics, nothing depends on the other prompts of the launch: bit-identical run to run, and a prompt alone
 * gives the bits it gives in company. The S weights of a prompt stay in LDS: samples <= 4096 (the largest fan the
 * README measures); above that MMT_ERR_UNSUPPORTED, nothing is re-read from memory.
 * MMT_ERR_INVALID before any launch: batch < 0, samples < 1, count outside 0..8, j0 < 0, j1 < j0, a NaN threshold,
 * lp_stride[i] < j1, batch * samples >= 2^31, a null pointer with batch > 0. batch == 0 launches nothing. */
int mmt_resample(void* stream, int32_t batch, int32_t samples, int32_t count, const float* const* logprob,
                 const int64_t* lp_stride, int32_t j0, int32_t j1, double* logw, double* log_evidence,
                 double ess_threshold, uint64_t seed, uint32_t pos, int32_t* ancestors, int32_t* resampled);

/* mmt_fanout_gather: the tails of a fan-out run follow their ancestors. For every tail of the run's fan buffer plan
 * (per (layer, modality) the self-attention tail, per (layer, cross modality, KV stream) the cross tail) the first
 * npos positions of row r of dst_fan become those of row ancestors[r] of src_fan: one gather kernel with 16-byte
 * accesses over a segment table the engine takes from its own plan, up to 64 segments per launch. Whole positions
 * are copied (the K, Q and V thirds of a self-attention row are contiguous); what no later step reads, the Q third
 * and positions >= npos, is unspecified in dst. The compact per-step scratch at the front of the buffer is not
 * copied, and the run state (next position, n0, samples) is left as it is: the next mmt_decode_fanout_step is
 * simply handed dst_fan. An ancestor outside 0..batch*samples-1 is read as the row itself.
 * Refusals, each before any launch: a null pointer, src_fan == dst_fan, buffers not 16-byte aligned
 * (MMT_ERR_INVALID); batch / samples / n0 / max_new that are not the run in progress, or no run (MMT_ERR_STATE);
 * npos != next position - n0 (MMT_ERR_INVALID). */
int mmt_fanout_gather(mmt_ctx* ctx, void* stream, int32_t batch, int32_t samples, int32_t n0, int32_t max_new,
                      int32_t npos, const int32_t* ancestors, const void* src_fan, void* dst_fan);

/* Forecast distributions of rollouts. A rollout returns paths; a forecast needs, per future step, the distribution
 * of the next token given the prompt: the average, over a prompt's paths, of the law each path draws its token
 * from, the paths weighted by their evidence. mmt_forecast_multi computes that mixture for one generated step,
 * mmt_pmf_stats reduces stored mixtures to summaries. Both need no context.
 *
 * mmt_forecast_multi: `count` problems (the heads of the step) over `batch` prompts of `samples` rows each, row
 * r = b * samples + s. V, logits, row_stride, temperature, top_k, top_p are HOST arrays of `count` entries with
 * mmt_sample_multi's meaning. Per problem the fp32 output row of prompt b is pmf[p] + b * pmf_stride[p]
 * (pmf_stride >= V: column j of a [B, N, V] tensor is written in place, stride N * V), and, where given,
 * ess[p][b] (fp64) and live[p][b] (int32); the arrays ess / live and their entries may be NULL. Weights in
 * mmt_resample's form: `wcount` <= 8 log-probability matrices (HOST arrays logprob / lp_stride), the column range
 * [j0, j1), logw fp64 [batch * samples] (nullable); logw_out (nullable, fp64 [batch * samples], not overlapping logw)
 * receives rule 2's a_s, so a loop that hands them back as the next step's logw folds one column per step and forms,
 * bit for bit, the serial sum over all of them. scratch: mmt_forecast_scratch_bytes(count, batch, samples)
 * bytes of device memory, 16-byte aligned, its contents unspecified before and after.
 * The rule, per problem p and prompt b:
 *   1. row law. For every row r, steps 1 - 4 of mmt_sample's rule with problem p's settings, by the sampler's own
 *      device code: z, m, the threshold key K of top-k then top-p, e_i = exp(z_i - m) (fp32, 1 at the maximum) on the
 *      kept set and 0 elsewhere, S_r their fp64 sum over the sampler's tree. The law is P_r(i) = e_i / S_r.
 *      temperature == 0: the point mass on the lowest index among the maxima of the raw logits (S_r = 1). A row with
 *      no finite logit has no law and is dead in this problem.
 *   2. path weight, mmt_resample's rules 1 - 2: a_s = logw[r] + the columns j0..j1-1 of the matrices (serial fp64 sum,
 *      NaN as -inf); mx = max over the rows that are not dead; d_s = (float)(a_s - mx); w_s = 1 where d_s == 0, else
 *      expf(d_s); w_s = 0 for dead rows and for a_s = -inf. W = sum w_s and Q = sum w_s^2 in fp64 over
 *      mmt_resample's tree; ess = W^2 / Q; live = #{ w_s > 0 }. Without weights (wcount == 0 and logw == NULL)
 *      w_s = 1 on every row that is not dead, W = Q = ess = live.
 *   3. mixture. c_s = (double) w_s / S_r; q(i) = (sum over s of e_i c_s) / W: fp64, one fused multiply-add per row,
 *      the rows of a prompt in sixteen consecutive blocks of ceil(samples / 16), each summed in row order, the sixteen
 *      partial sums added left to right; q is rounded to fp32 once. live == 0 gives an all-zero row and ess 0.
 * No float atomics: a launch is bit-identical run to run, a prompt launched alone (same samples) gives the bits it
 * gives in company, and so does a problem. Nothing outside the V columns of a pmf row is written.
 * Launches: one over (rows, problems) for the row laws (a second one for problems with V > 8192, the sampler's
 * re-read variant), with weights one over (prompts, problems), one over (prompts x 64-column chunks, problems);
 * more than 8 problems go in chunks of 8. With weights samples <= 4096 (the weights of a prompt stay in LDS);
 * without, any.
 * MMT_ERR_INVALID before any launch, nothing written: count < 0, batch < 0, samples < 1, batch * samples >= 2^31,
 * wcount outside 0..8, j0 < 0, j1 < j0; with count > 0 a null V / logits / row_stride / temperature / top_k /
 * top_p / pmf / pmf_stride array; per problem mmt_sample's refusals, pmf_stride < V, a null logits / pmf with
 * batch > 0; with wcount > 0 and j1 > j0 a null logprob / lp_stride or entry, lp_stride < j1; with batch > 0 a
 * null, misaligned or undersized scratch; logw_out without weights or equal to logw.
 * MMT_ERR_UNSUPPORTED: V > 2^20; with weights samples > 4096 or
 * count > 65535. count == 0 or batch == 0 launches nothing. mmt_forecast_scratch_bytes returns -1 for arguments
 * the entry refuses. */
int64_t mmt_forecast_scratch_bytes(int32_t count, int32_t batch, int32_t samples);
int mmt_forecast_multi(void* stream, int32_t count, int32_t batch, int32_t samples, const int32_t* V,
                       const float* const* logits, const int64_t* row_stride, const float* temperature,
                       const int32_t* top_k, const float* top_p, float* const* pmf, const int64_t* pmf_stride,
                       int32_t wcount, const float* const* logprob, const int64_t* lp_stride, int32_t j0, int32_t j1,
                       const double* logw /* nullable */, double* logw_out /* nullable */,
                       double* const* ess /* nullable, entries nullable */,
                       int32_t* const* live /* nullable, entries nullable */, void* scratch, int64_t scratch_bytes);

/* mmt_pmf_stats: summaries of stored pmf rows, `count` problems over the same `rows`, grid (rows, problems). Per
 * problem (HOST arrays): V, the fp32 pmf (row r at pmf[p] + r * pmf_stride[p]), values (device fp64 [V],
 * non-decreasing in token order; the array and its entries nullable), is_percent (nullable: all 0), origin (device
 * int64, row r's at origin[p][r * origin_stride[p]]; nullable), stats (device fp64 [rows, 8]), qtok (device int32
 * [rows, nq]). levels: `nq` <= 16 HOST fp64 values in (0, 1).
 * Everything is a function of the fp32 row as stored, in fp64; an entry that is not > 0 holds no mass. Sums run in
 * vocabulary order over the sampler's tree (thread t of 256 owns the c = ceil(V / 256) | 1 elements from t c).
 *   stats[0] T = sum q          stats[1] entropy -sum (q/T) ln (q/T), nats
 *   stats[2] mean sum (q/T) v   stats[3] variance sum (q/T) (v - mean)^2
 *   stats[4..6] p_down, p_flat, p_up: the mass / T of the tokens whose direction sign is -1 / 0 / +1, the sign of
 *               v_i for a percent series (origin is not read) and of v_i - v[origin] for a value series (the
 *               reference's _get_direction_sign against the origin token)
 *   stats[7] the largest q / T
 *   qtok[k] the first token with mass whose inclusive prefix sum reaches levels[k] * T (should rounding leave
 *           none, the last token with mass)
 * Without values stats[2..6] are NaN (the quantiles are those of the token index); an origin outside 0..V-1, or
 * none for a value series, gives NaN in stats[4..6] and nothing is read out of range. A row with T == 0 gives
 * stats[0] = 0, NaN in stats[1..7] and qtok -1.
 * MMT_ERR_INVALID before any launch: count < 0, rows < 0, nq outside 0..16, a level outside (0, 1) or NaN, a null
 * V / pmf / pmf_stride / stats array, qtok null with nq > 0, origin without origin_stride, V < 1, pmf_stride < V,
 * a null pmf / stats / qtok entry with rows > 0; MMT_ERR_UNSUPPORTED for V > 2^20. */
int mmt_pmf_stats(void* stream, int32_t count, int32_t rows, const int32_t* V, const float* const* pmf,
                  const int64_t* pmf_stride, const double* const* values /* nullable, entries nullable */,
                  const int32_t* is_percent /* nullable */, const int64_t* const* origin /* nullable */,
                  const int64_t* origin_stride, int32_t nq, const double* levels, double* const* stats,
                  int32_t* const* qtok);

/* Horizon forecasts. mmt_forecast_multi gives the law of the token at new step j: for a percent series the law of one
 * step's change. Where the series stands after j steps, its quantiles there and whether it touched a barrier by then
 * depend on each path's own history. mmt_horizon_stats computes them from the finished paths and their log-weights,
 * in one call after the loop. No context.
 *
 * `count` problems (modalities) over `batch` prompts of `samples` rows each, row r = b * samples + s, `steps` new
 * tokens per row. Per problem (HOST arrays): V; tok (device int64, token j of row r at tok[p] + r * tok_stride[p] + j:
 * the caller points at the first new column of a sequence buffer); values (device fp64 [V], required); is_percent
 * (nullable: all 0); origin (device int64, row r's at origin[p][r * origin_stride[p]]; required for a value series,
 * not read for a percent series). Shared by all problems: logw fp64 [batch * samples] (nullable), `nq` <= 16 HOST
 * levels in (0, 1), `nb` <= 8 barriers per problem (HOST array of HOST arrays, every entry finite and non-zero).
 * Outputs per problem: stats fp64 [batch, steps, 12], qval fp64 and qrow int32 [batch, steps, nq], hit fp64 [batch,
 * steps, nb], ess fp64 [batch], live int32 [batch]; qval / qrow / hit may be NULL when nq / nb is 0, the arrays ess /
 * live and their entries may be NULL. scratch: mmt_horizon_scratch_bytes(count, batch, samples, steps) bytes of
 * device memory, 16-byte aligned, its contents unspecified before and after.
 * The rule, per problem and prompt b, with v = values:
 *   1. path quantities, per row and step in fp64, serially in step order, every line ONE IEEE operation (nothing is
 *      contracted into a multiply-add). Percent series: c = v[t_j] / 100; u = 1 + c; g_j = g_{j-1} * u (g_{-1} = 1);
 *      e = g_j - 1; x_j = e * 100. Value series: x_j = v[t_j] - v[origin]. Running extremes including the origin:
 *      hi_j = max(hi_{j-1}, x_j), lo_j = min(lo_{j-1}, x_j), hi_{-1} = lo_{-1} = 0. Step direction d_j: the sign of
 *      v[t_j] for a percent series, of v[t_j] - v[t_{j-1}] for a value series with t_{-1} the origin (the reference's
 *      _get_direction_sign against each path's own previous token). A row is dead in the problem when one of its
 *      tokens is outside 0..V-1, when it is a value series and its origin is outside 0..V-1, or when some x_j is not
 *      finite. Nothing is read out of range.
 *   2. weights, mmt_resample's rules 1 - 2 as in mmt_forecast_multi: a_s = logw[r] (NaN counts as -inf); mx = max over
 *      the rows that are not dead; w_s = 1 where (float)(a_s - mx) == 0, else expf of it; dead rows and a_s = -inf
 *      get 0. W = sum w_s and Q = sum w_s^2 in fp64 over mmt_resample's tree; ess = W^2 / Q; live = #{ w_s > 0 }.
 *      Without logw w_s = 1 on every row that is not dead.
 *   3. stats[b, j, 0..11], fp64 sums over the prompt's rows in row order over the same tree:
 *        [0] mean sum w x / W            [1] variance sum w (x - mean)^2 / W
 *        [2..4] the mass / W of x < 0, x == 0, x > 0 (direction over the horizon)
 *        [5..7] the mass / W of d = -1, 0, +1 (step direction)
 *        [8] mean of hi   [9] mean of lo   [10], [11] the smallest and the largest x over the rows with w > 0
 *   4. quantiles: the rows with w > 0 in the order (x_j, s) ascending; qrow[k] is the local path index s of the first
 *      row whose inclusive fp64 prefix sum of w in that order reaches levels[k] * W (one fp64 product; should
 *      rounding leave none, the last row with weight), qval[k] that row's x_j, bit for bit.
 *   5. barriers: hit[b, j, k] = sum w [hi_j >= u] / W for u > 0 and sum w [lo_j <= u] / W for u < 0: the probability
 *      of having touched the barrier by step j, which does not decrease in j.
 * live == 0 gives NaN stats, NaN qval, qrow -1, NaN hit, ess 0. No float atomics: bit-identical run to run; a prompt
 * launched alone (same samples) gives the bits it gives in company, and so does a problem. Nothing outside the named
 * outputs is written.
 * Launches: one over (rows / 256, problems) for rule 1, one over (prompts x steps, problems) for the rest (the
 * weights of a prompt and the keys of one step in LDS, 56 KiB at 4096 rows); more than 8 problems go in chunks of 8.
 * MMT_ERR_INVALID before any launch, nothing written: a negative count, batch or steps; samples < 1; batch * samples
 * >= 2^31; nq outside 0..16 or nb outside 0..8; a level outside (0, 1) or NaN; a barrier that is zero, NaN or
 * infinite; V < 1; tok_stride < steps; a null required array or entry; a value series without origin; a scratch that
 * is null, misaligned or undersized. MMT_ERR_UNSUPPORTED: V > 2^20, samples > 4096, batch * steps >= 2^31. count,
 * batch or steps of 0 launches nothing. mmt_horizon_scratch_bytes returns -1 for arguments the entry refuses. */
int64_t mmt_horizon_scratch_bytes(int32_t count, int32_t batch, int32_t samples, int32_t steps);
int mmt_horizon_stats(void* stream, int32_t count, int32_t batch, int32_t samples, int32_t steps, const int32_t* V,
                      const int64_t* const* tok, const int64_t* tok_stride, const double* const* values,
                      const int32_t* is_percent /* nullable */, const int64_t* const* origin,
                      const int64_t* origin_stride, const double* logw /* nullable */, int32_t nq,
                      const double* levels, int32_t nb, const double* const* barriers, double* const* stats,
                      double* const* qval, int32_t* const* qrow, double* const* hit,
                      double* const* ess /* nullable, entries nullable */,
                      int32_t* const* live /* nullable, entries nullable */, void* scratch, int64_t scratch_bytes);

/* Scores of horizon forecasts. mmt_horizon_stats says where the paths of a prompt stand after j steps;
 * mmt_horizon_score sets that against the series that was realised: per (prompt, step) proper scores of the weighted
 * sample and of the forecast mmt_horizon_stats made of it, per step tables that accumulate over the calls of a
 * backtest. No context.
 *
 * Paths: count, batch, samples, steps, V, tok, tok_stride, values, is_percent, origin, origin_stride, logw, nq, levels,
 * nb, barriers as mmt_horizon_stats takes them. The realised series, one row per prompt: real (per problem a device
 * int64 pointer, token j of prompt b at real[p] + b * real_stride[p] + j) and, required for a value series,
 * real_origin (prompt b's at real_origin[p][b * real_origin_stride[p]]). The forecast, read and never recomputed:
 * stats fp64 [batch, steps, 12], qval fp64 [batch, steps, nq], hit fp64 [batch, steps, nb], as a mmt_horizon_stats call
 * on the same paths, weights, levels and barriers wrote them (qval / hit may be NULL when nq / nb is 0): the pointwise
 * scores are a function of the forecast the caller holds. bins in 1..64. Outputs per problem: sc fp64 [batch, steps, 8]
 * (the array and its entries nullable: the records then live in the scratch), pin fp64 [batch, steps, nq], bs fp64
 * [batch, steps, nb], and the tables agg fp64 [steps, 10], aggq fp64 [steps, nq, 2], aggb fp64 [steps, nb, 3], pit
 * fp64 [steps, bins] (pin / aggq and bs / aggb may be NULL when nq / nb is 0). scratch:
 * mmt_horizon_score_scratch_bytes(count, batch, samples, steps) bytes of device memory, 16-byte aligned, its contents
 * unspecified before and after.
 * The rule, per problem, prompt b and step j:
 *   1. the realised row is walked by rule 1 of mmt_horizon_stats (the same device function): x*, hi*, lo*, d* per
 *      step. A realised row that rule 1 calls dead is dead at every step, and so is a prompt without a row with weight
 *      (live == 0). A dead (b, j) has NaN in every sc / pin / bs field and enters no table.
 *   2. weights: rule 2 of mmt_horizon_stats, unchanged: w_s, W (the same sum over the same tree, so the same bits)
 *      and the rows with weight.
 *   3. CRPS, the integral of (F - [x* <= t])^2 over t, piecewise: the n rows with weight in the order (x_j, s) of rule
 *      4; P_m the inclusive fp64 prefix of w through place m over the chunk tree of that rule. For each gap between
 *      the places m and m + 1, one IEEE operation each: a = x_(m); b = x_(m+1); s = min(b, max(a, x*)); F = P_m / W;
 *      F2 = F * F; G = 1 - F; G2 = G * G; lo = (s - a) * F2; up = (b - s) * G2; term = lo + up. The terms are summed in
 *      place order over the tree (thread t owns the c = ceil(samples / 256) | 1 places from t c, a gap belonging to
 *      its lower place: serial sum from 0, shift scan over the lanes, the four wave totals left to right). The tail,
 *      x_(1) - x* when x* < x_(1), x* - x_(n) when x* > x_(n), else 0, is added to that sum last. Every term is
 *      non-negative; the CRPS is 0 when every x equals x* and |x_1 - x*| at one row.
 *   4. PIT (mid): (L + 0.5 * E) / W with L = sum w [x < x*] and E = sum w [x == x*], both in row order over the tree;
 *      h = 0.5 * E; n = L + h; PIT = n / W. The comparisons are exact: x* comes from the walk that made x.
 *   5. sc[b, j, 0..7]: [0] x*  [1] CRPS  [2] PIT  [3] stats[0] - x*, the error of the mean  [4] the entry of
 *      stats[2..4] that the sign of x* selects  [5] the entry of stats[5..7] that d* selects  [6] hi*  [7] lo*
 *   6. pin[b, j, k] = (x* - q) * (levels[k] - [x* < q]), q = qval[b, j, k]: one subtraction each, then the product.
 *   7. bs[b, j, k] = (hit[b, j, k] - o)^2, o = [hi* >= u] for a barrier u > 0 and [lo* <= u] for u < 0.
 *   8. tables, a function of the records, the forecast and d*: every cell is a serial fp64 sum from 0 over the live
 *      (b, j) of step j, b ascending, so counts are exact.
 *      agg[j, .]: [0] scored prompts  [1] sum CRPS  [2] sum |x*| (the CRPS of a "no change" forecast: skill = 1 -
 *        [1] / [2])  [3] sum |sc[3]|  [4] sum sc[3]^2  [5] sum sc[4]  [6] sign hits: the largest of stats[2..4], the
 *        lowest index on ties, is the entry the sign of x* selects  [7] sum sc[5]  [8] step-direction hits, the same
 *        on stats[5..7] and d*  [9] sum stats[1], the mean forecast variance, to set against [4]
 *      aggq[j, k, .]: [0] sum pin  [1] #{ x* <= q }
 *      aggb[j, k, .]: [0] sum bs  [1] sum hit  [2] #{ o = 1 }
 *      pit[j, min(bins - 1, floor(PIT * bins))] (one fp64 product) counts the prompt.
 *      accumulate == 0 writes the tables; otherwise each cell is added, with one fp64 addition, to what the buffer
 *      holds.
 * No float atomics: bit-identical run to run; a prompt launched alone (same samples) gives the sc / pin / bs it gives
 * in company, and so does a problem. Nothing outside the named buffers is written.
 * Launches, per chunk of 8 problems: one over ((batch samples + batch) / 256, problems) for rule 1 on the paths and
 * the realised rows, one over (prompts x steps, problems) for the records (the weights of a prompt and the keys of one
 * step in LDS, 56 KiB at 4096 rows), one over (steps, problems) for the tables, a thread per cell.
 * MMT_ERR_INVALID before any launch, nothing written: what mmt_horizon_stats refuses so, with batch * samples + batch
 * >= 2^31 in place of its bound on batch * samples; bins outside 1..64; real_stride < steps; a null required array or
 * entry; a value series without origin or real_origin. MMT_ERR_UNSUPPORTED: V > 2^20, samples > 4096, batch * steps >=
 * 2^31. count, batch or steps of 0 launches nothing and writes nothing. mmt_horizon_score_scratch_bytes returns -1
 * for arguments the entry refuses. */
int64_t mmt_horizon_score_scratch_bytes(int32_t count, int32_t batch, int32_t samples, int32_t steps);
int mmt_horizon_score(void* stream, int32_t count, int32_t batch, int32_t samples, int32_t steps, const int32_t* V,
                      const int64_t* const* tok, const int64_t* tok_stride, const double* const* values,
                      const int32_t* is_percent /* nullable */, const int64_t* const* origin,
                      const int64_t* origin_stride, const int64_t* const* real, const int64_t* real_stride,
                      const int64_t* const* real_origin, const int64_t* real_origin_stride,
                      const double* logw /* nullable */, int32_t nq, const double* levels, int32_t nb,
                      const double* const* barriers, const double* const* stats, const double* const* qval,
                      const double* const* hit, int32_t bins, int32_t accumulate,
                      double* const* sc /* nullable, entries nullable */, double* const* pin, double* const* bs,
                      double* const* agg, double* const* aggq, double* const* aggb, double* const* pit, void* scratch,
                      int64_t scratch_bytes);

/* Joint horizon forecasts. mmt_horizon_stats gives the marginal of each series after j steps; the paths of a joint
 * rollout also carry the dependence between the series. mmt_horizon_joint reads it off the same paths: per basket
 * (a position sum_p coef[k][p] x^(p) in the series) the moments, sign masses, quantiles, tail means and barrier hits
 * of its value, per pair of series their covariance, correlation and the tables of their signs. No context.
 *
 * Paths: count, batch, samples, steps, V, tok, tok_stride, values, is_percent, origin, origin_stride, logw, nq, levels
 * as mmt_horizon_stats takes them; count in 1..8 (one chunk), the caller passes only the series that take part.
 * `nbk` <= 8 baskets: HOST fp64 coef[nbk][count], every entry finite, each basket with a non-zero entry; one `nb` <= 8
 * for all baskets, HOST barriers[nbk][nb], finite and non-zero. `npair` <= 28 pairs: HOST int32 pairs[npair][2],
 * problem indices p != q in 0..count-1. Outputs (HOST arrays of device pointers): per basket bstats fp64 [batch, steps,
 * 9], bqval fp64, bqrow int32 and btail fp64 [batch, steps, nq], bhit fp64 [batch, steps, nb]; per pair pstats fp64
 * [batch, steps, 22]; ess fp64 [batch] and live int32 [batch] (device, nullable). The arrays of a kind whose count
 * (nbk, nq, nb, npair) is 0 may be NULL. scratch: mmt_horizon_joint_scratch_bytes(count, batch, samples, steps, nbk)
 * bytes of device memory, 16-byte aligned, its contents unspecified before and after.
 * The rule, per prompt b, every line ONE IEEE fp64 operation (nothing is contracted into a multiply-add):
 *   1. every problem is walked by rule 1 of mmt_horizon_stats (the same device function): x, hi, lo, d bit for bit.
 *      Basket k of row r at step j: y = 0.0; for p = 0..count-1 ascending t = coef[k][p] * x_j^(p); y = y + t (no
 *      coefficient is skipped). hi^y_j = max(hi^y_{j-1}, y_j), lo^y_j = min(lo^y_{j-1}, y_j), both from 0. A row is dead
 *      for the whole call when it is dead in any problem of the call or when some y is not finite: a cross-series
 *      statistic needs every series of the row.
 *   2. weights: rule 2 of mmt_horizon_stats over the rows that are not dead: w_s, W, Q, ess, live. Where no row is
 *      dead they are bit for bit what mmt_horizon_stats writes.
 *   3. bstats[b, j, 0..8], sums in row order over the same tree: [0] mean of y  [1] variance about that mean (second
 *      pass, w * (dv * dv))  [2..4] the mass / W of y < 0, y == 0, y > 0  [5] mean of hi^y  [6] mean of lo^y  [7], [8]
 *      the smallest and the largest y over the rows with weight.
 *   4. bqval / bqrow: rule 4 of mmt_horizon_stats on the order (y_j, s).
 *   5. btail, the mean of y below each quantile (the expected shortfall): m the place of the quantile row in that
 *      order; P and A the inclusive prefixes of w and of w y (one product per row) through place m - 1 over the tree of
 *      rule 4's prefix (both 0 at m = 0); target = levels[k] * W; rem = target - P; t = rem * y_(m); num = A + t; btail =
 *      num / target. A caller mirrors the coefficients for the upper tail.
 *   6. bhit: rule 5 of mmt_horizon_stats on hi^y / lo^y.
 *   7. pstats[b, j, 0..21] of pair (p, q): m_p, m_q rule 3's means (sum w x / W). Per row a = x_p - m_p, c = x_q - m_q
 *      and the terms w * (a * a), w * (c * c), w * (a * c): the product of the deviations first, then the weight, as
 *      rule 3 of mmt_horizon_stats forms its variance. Summed in row order over the tree.
 *        [0] cov = sum w a c / W   [1] corr = cov / (sqrt(var_p) * sqrt(var_q)), NaN when that denominator is 0, not
 *        clamped   [2] var_p   [3] var_q   [4..12] the mass / W of (sign x_p, sign x_q) at 3 (s_p + 1) + (s_q + 1)
 *        [13..21] the same of the step directions (d_p, d_q)
 *      Where no row is dead var_p is bit for bit stats[1] of mmt_horizon_stats for problem p.
 *   8. live == 0 gives NaN in every fp64 output, bqrow -1, ess 0.
 * No float atomics: bit-identical run to run; a prompt launched alone (same samples) gives the bits it gives in
 * company; a basket or a pair gives the same bits whatever other baskets and pairs are in the call. Nothing outside
 * the named outputs is written.
 * Launches: one over rows / 256 for rule 1 and the baskets of each row, one over (prompts x steps, nbk) (the weights of
 * a prompt and the keys of one step in LDS, 56 KiB at 4096 rows), one over (prompts x steps, npair) (the weights in
 * LDS, 16 KiB).
 * MMT_ERR_INVALID before any launch, nothing written: what mmt_horizon_stats refuses so; nbk outside 0..8 or npair
 * outside 0..28; a coefficient that is NaN or infinite; a basket of zeros; a pair index outside 0..count-1 or p == q; an
 * output array or entry that is null while its count is not 0. MMT_ERR_UNSUPPORTED: count > 8, V > 2^20, samples >
 * 4096, batch * steps >= 2^31. nbk == 0 and npair == 0 together, or batch or steps of 0, launch nothing.
 * mmt_horizon_joint_scratch_bytes returns -1 for arguments the entry refuses. */
int64_t mmt_horizon_joint_scratch_bytes(int32_t count, int32_t batch, int32_t samples, int32_t steps, int32_t nbk);
int mmt_horizon_joint(void* stream, int32_t count, int32_t batch, int32_t samples, int32_t steps, const int32_t* V,
                      const int64_t* const* tok, const int64_t* tok_stride, const double* const* values,
                      const int32_t* is_percent /* nullable */, const int64_t* const* origin,
                      const int64_t* origin_stride, const double* logw /* nullable */, int32_t nq,
                      const double* levels, int32_t nbk, const double* coef, int32_t nb, const double* barriers,
                      int32_t npair, const int32_t* pairs, double* const* bstats, double* const* bqval,
                      int32_t* const* bqrow, double* const* btail, double* const* bhit, double* const* pstats,
                      double* ess /* nullable */, int32_t* live /* nullable */, void* scratch, int64_t scratch_bytes);

/* Evaluation at every position. mmt_eval_direction scores the last position of every window; the evaluation forward
 * has written the logits of all batch * T rows. mmt_eval_positions scores every row with t >= t_begin: direction,
 * log score and what a calibration check of the head's probabilities needs, then reduces the rows to tables. No
 * context.
 *
 * `count` problems (the modalities) over the same `batch` and `T`. Per problem (HOST arrays): V; logits (device
 * fp32 [batch, T, V], row (b, t) at logits[p] + (b T + t) V); xb and yb (device int64 [batch, T]: the token at
 * position t and the token that followed it, as get_batch makes them); values (device fp64 [V]; the array and its
 * entries nullable); is_percent (nullable: all 0). Outputs per problem: rec (device fp64 [batch, T, 8]; the array
 * and its entries nullable: the records then live in the scratch), pos fp64 [T, 8], rel fp64 [3, bins, 3], pit
 * fp64 [bins]. scratch: mmt_eval_positions_scratch_bytes(count, batch, T, bins) bytes of device memory, 16-byte
 * aligned, its contents unspecified before and after.
 * Stage 1, the record of row (b, t), t >= t_begin. The law of the row is mmt_sample's at temperature 1, top_k 0,
 * top_p 1, by the sampler's own device code: z the logit, NaN as -inf; m = max z; e_i = expf(z_i - m) in fp32, 1 at
 * the maximum; S the fp64 sum of the e_i over the sampler's tree (thread t of 256 owns the c = ceil(V / 256) | 1
 * elements from t c: serial sum, shift scan over the lanes, the four wave totals left to right); P(i) = e_i / S. A
 * mass below is the fp64 sum over that same tree of the e_i of a class (the other leaves zeroed), divided by S once.
 * The direction sign of token i is that of values[i] for a percent series and of values[i] - values[xb] (one fp64
 * subtraction) for a value series: the reference's _get_direction_sign, mmt_pmf_stats' stats[4..6] with origin xb.
 *   rec[0] the log-probability of yb: the fp32 value mmt_score_multi writes for that row and token, widened
 *   rec[1..3] p_down, p_flat, p_up: the masses of the tokens whose sign is -1 / 0 / +1
 *   rec[4] the mid-PIT in token order: (mass of { i < yb } before the division + 0.5 e_yb) / S
 *   rec[5] the rank of yb, #{ i : z_i > z_yb }, exact comparisons: 0 is the arg-max group
 *   rec[6] the predicted sign: that of the lowest index among the maxima of the raw logits (NaN as -inf), the token
 *          mmt_eval_direction predicts
 *   rec[7] the realised sign: that of yb
 * Without values rec[1..3], rec[6] and rec[7] are NaN. A row with no finite logit, or with xb or yb outside 0..V-1
 * (neither is then used as an index), is dead: its eight fields are NaN. Records of rows with t < t_begin are not
 * written.
 * Stage 2, the tables, a function of the records alone. A row is live when rec[5] is not NaN and has a direction
 * when rec[6] is not NaN. Every sum is serial in fp64 from 0; counts are therefore exact.
 *   pos[t, k], over the rows of position t, b ascending (zero for t < t_begin):
 *     [0] live rows                    [1] wins, rec[6] == rec[7]      [2] losses, rec[6] != rec[7]
 *     [3] certainty: the sum of the mass rec[1..3] the predicted sign selects (the reference's certainty)
 *     [4] the sum of -rec[0]           [5] top-1 hits, rec[5] == 0     [6] rows with a direction
 *     [7] the sum of the mass the realised sign selects
 *   rel[d, k, 0..2], d = 0, 1, 2 for down, flat, up: a row with a direction enters bin
 *     k = min(bins - 1, floor(P_d * bins)), P_d = rec[1 + d] (one fp64 product); the cell holds the count, the sum
 *     of P_d, and the number of rows whose realised sign is d - 1
 *   pit[k]: the live rows with k = min(bins - 1, floor(rec[4] * bins))
 * A rel or pit cell is the sum over t = t_begin..T-1 ascending of the position's own sum over b ascending.
 * accumulate == 0 writes the tables; otherwise each cell is added, with one fp64 addition, to what the buffer
 * holds. No float atomics: a launch is bit-identical run to run, and a problem gives in company the bits it gives
 * alone. Nothing outside the named buffers is written.
 * Launches, per chunk of 8 problems: one over (batch (T - t_begin), problems) for the records (a second one for the
 * problems with V > 8192, the sampler's re-read variant), one over (T, problems) for the positions, one over
 * (problems) for the reliability and PIT cells.
 * MMT_ERR_INVALID before any launch, nothing written: count, batch or T negative; t_begin outside 0..T; bins
 * outside 1..64; batch * T >= 2^31; with count > 0 a null V / logits / xb / yb / pos / rel / pit array; V < 1; with
 * batch > 0 and t_begin < T a null logits / xb / yb / pos / rel / pit entry; with batch > 0 a null, misaligned or
 * undersized scratch. MMT_ERR_UNSUPPORTED for V > 2^20. count == 0, batch == 0 and t_begin == T launch nothing and
 * write nothing. mmt_eval_positions_scratch_bytes returns -1 for arguments the entry refuses. */
int64_t mmt_eval_positions_scratch_bytes(int32_t count, int32_t batch, int32_t T, int32_t bins);
int mmt_eval_positions(void* stream, int32_t count, int32_t batch, int32_t T, int32_t t_begin, int32_t bins,
                       int32_t accumulate, const int32_t* V, const float* const* logits,
                       const int64_t* const* xb, const int64_t* const* yb,
                       const double* const* values /* nullable, entries nullable */,
                       const int32_t* is_percent /* nullable */,
                       double* const* rec /* nullable, entries nullable */, double* const* pos,
                       double* const* rel, double* const* pit, void* scratch, int64_t scratch_bytes);

/* Calibrated temperatures. Every head is sampled from softmax(logits / temperature); mmt_eval_temperatures scores
 * the rows mmt_eval_positions scores under K temperatures from one read of each row, and reduces them to what a fit
 * of the temperature needs: per temperature the summed log score, and the reliability tables of the direction
 * masses. No context, no knobs.
 *
 * `count` problems over the same `batch`, `T`, `t_begin`, `bins`, `accumulate` and the same K temperatures
 * (`temperatures`: a HOST array of K floats, 1 <= K <= 32, every one finite and > 0, strictly ascending). Per
 * problem (HOST arrays) V, logits, xb, yb, values and is_percent are mmt_eval_positions' own. Outputs per problem:
 * rec (device fp64 [batch, T, K, 4]; the array and its entries nullable: the records then live in the scratch),
 * sum fp64 [K, 2], rel fp64 [K, 3, bins, 3]. scratch: mmt_eval_temperatures_scratch_bytes(count, batch, T, bins, K)
 * bytes of device memory, 16-byte aligned, its contents unspecified before and after.
 * Stage 1, the record of row (b, t) and temperature k, t >= t_begin. The law is mmt_sample's at temperature
 * temperatures[k], top_k 0, top_p 1, by the sampler's own device functions: inv_t = 1.0f / temperatures[k] (one
 * fp32 division on the host); z_i = logit_i * inv_t (one fp32 multiply), NaN as -inf; m = max z (the scaled maximum
 * of the raw row: inv_t > 0 and rounding is monotone); e_i = expf(z_i - m), 1 at the maximum; S the fp64 sum of the
 * e_i over the sampler's tree (mmt_eval_positions, stage 1). A mass is the sum over that tree of the e_i of a
 * direction class (the other leaves zeroed), divided by S once; the classes are mmt_eval_positions'.
 *   rec[0] the log-probability of yb: (z_yb - m) - log S rounded to fp32 once, widened; -inf where z_yb is -inf
 *   rec[1..3] p_down, p_flat, p_up; NaN without values
 * So at temperatures[k] == 1.0f the four fields are bit for bit mmt_eval_positions' rec[0..3], and for any
 * temperature rec[0] is bit for bit the log-probability mmt_sample writes when it draws yb at that temperature,
 * and what mmt_score_multi gives on logits * inv_t. A row is dead where mmt_eval_positions calls it dead (no finite
 * logit, or xb or yb outside 0..V-1, neither then used as an index), for every k alike: its K x 4 fields are NaN.
 * Records of rows with t < t_begin are not written.
 * Stage 2, the tables, a function of the records and of the realised sign (that of yb, mmt_eval_positions'
 * rec[7], taken again from values, xb and yb). A row is live when rec[0] is not NaN and has a direction when
 * rec[1] is not NaN. Every sum is serial in fp64 from 0; counts are therefore exact.
 *   sum[k, 0] live rows                 sum[k, 1] the sum of -rec[0]
 *   rel[k, d, j, 0..2], d = 0, 1, 2 for down, flat, up: a row with a direction enters bin
 *     j = min(bins - 1, floor(P_d * bins)), P_d = rec[1 + d]; the cell holds the count, the sum of P_d, and the
 *     number of rows whose realised sign is d - 1
 * A cell is the sum over t = t_begin..T-1 ascending of the position's own sum over b ascending. accumulate == 0
 * writes the tables; otherwise each cell is added, with one fp64 addition, to what the buffer holds. No float
 * atomics: a launch is bit-identical run to run, and a problem gives in company the bits it gives alone. Nothing
 * outside the named buffers is written.
 * Launches, per chunk of 8 problems: one over (batch (T - t_begin), problems) for the records (a second one for the
 * problems with V > 8192, the sampler's re-read variant), one over (T - t_begin, K, problems) for the positions, one
 * over (ceil(K (2 + 9 bins) / 256), problems) for the cells.
 * MMT_ERR_INVALID before any launch, nothing written: what mmt_eval_positions refuses (count, batch or T negative;
 * t_begin outside 0..T; bins outside 1..64; batch * T >= 2^31; with count > 0 a null V / logits / xb / yb / sum /
 * rel array; V < 1; with batch > 0 and t_begin < T a null logits / xb / yb / sum / rel entry; with batch > 0 a null,
 * misaligned or undersized scratch); K outside 1..32; a null temperatures; a temperature that is not finite, not
 * > 0 or not above its predecessor. MMT_ERR_UNSUPPORTED for V > 2^20. count == 0, batch == 0 and t_begin == T
 * launch nothing and write nothing. mmt_eval_temperatures_scratch_bytes returns -1 for arguments the entry
 * refuses. */
int64_t mmt_eval_temperatures_scratch_bytes(int32_t count, int32_t batch, int32_t T, int32_t bins, int32_t K);
int mmt_eval_temperatures(void* stream, int32_t count, int32_t batch, int32_t T, int32_t t_begin, int32_t bins,
                          int32_t accumulate, int32_t K, const float* temperatures, const int32_t* V,
                          const float* const* logits, const int64_t* const* xb, const int64_t* const* yb,
                          const double* const* values /* nullable, entries nullable */,
                          const int32_t* is_percent /* nullable */,
                          double* const* rec /* nullable, entries nullable */, double* const* sum,
                          double* const* rel, void* scratch, int64_t scratch_bytes);

/* failure detection (the reference's guard is the NaN check on eval losses,
 * main.py:606): byte offset in the workspace of two int32 bitmasks (the same for every batch size;
 * the query never touches the workspace plan of a pending backward or decode). The
 * loss kernel sets bit i of both when modality i's mean CE is NaN or Inf; word 0 is cleared by
 * every mmt_forward with targets (the last forward's flags), word 1 only by the caller (sticky
 * since the caller last cleared it; zero it when the workspace is allocated). Read them when the
 * host syncs anyway; no kernel ever traps. */
int64_t mmt_loss_flag_offset(mmt_ctx* ctx, int32_t batch);

/* dropout (model.py:57/69, 87/91, 107/116, 134/151, 171; nn.Dropout(p) in training mode only):
 * masks are a counter hash of (seed, layer, modality, site, row, column) regenerated in the
 * backward, so nothing is stored. Sets the seed of the NEXT training forward (and its backward);
 * without a call the engine derives one from mmt_config.seed and a per-context counter. */
int mmt_set_dropout_seed(mmt_ctx* ctx, uint64_t seed);

/* backward of sum_i loss_grads[i] * loss_i through the last mmt_forward (same workspace/params).
 * grads: fp32 flat buffer of the active prefix (mmt_param_active_count elements) — OVERWRITTEN
 * (zeroed then accumulated); the never-used tail past it has no gradient (reference: .grad None). */
int mmt_backward(mmt_ctx* ctx, void* stream, const float* loss_grads, const float* params, float* grads,
                 void* workspace);
/* the same, split into stages (post-block, layer L-1 .. layer 0, embeddings) so a caller can
 * all-reduce each finished gradient range while the next stage computes (DP overlap). */
int32_t mmt_backward_stage_count(const mmt_ctx* ctx);
int mmt_backward_stage_range(const mmt_ctx* ctx, int32_t stage, int64_t* begin, int64_t* end);
int mmt_backward_stage(mmt_ctx* ctx, void* stream, int32_t stage, const float* loss_grads, const float* params,
                       float* grads, void* workspace);

/* fused AdamW over n elements (torch.optim.AdamW semantics, decoupled decay, bias correction) */
int mmt_adamw_step(mmt_ctx* ctx, void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int64_t n, int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay);

/* ---- guarded optimizer step: gradient clipping, non-finite skip and the step count on the device ----
 * One step of an optimizer over several flat tensors, with no device-to-host copy or sync anywhere:
 *     mmt_grad_sqsum (add = 0) on the first gradient, mmt_grad_sqsum (add = 1) on every other one,
 *     mmt_guard_finalize once, mmt_adamw_step_guarded on every (params, grads, moments) tuple,
 * all on one stream. The guard state is mmt_guard_state_bytes bytes of device memory, 16-byte aligned,
 * allocated once per optimizer and zeroed by the caller before its first step; struct mmt_guard_header
 * sits at offset 0, MMT_GUARD_SLOTS fp64 block partials follow it. The sum of squares is taken in fp64
 * in a fixed order (fixed grid, fixed trees, no float atomics): the norm is bit-identical run to run in
 * both training modes, agrees with the exact value to below one fp32 ulp whatever n is, and a finite
 * fp32 gradient never overflows it. */
#define MMT_GUARD_SLOTS 1024
struct mmt_guard_header {
  float norm;              /* global L2 norm of this step's gradients, (float)sqrt(fp64 sum of squares) */
  float coef;              /* the factor the step applies to every gradient element (1 without clipping) */
  int32_t ok;              /* 1: the guarded steps of this optimizer step apply; 0: they return untouched */
  int32_t reserved0;
  int64_t applied_steps;   /* steps applied so far: the t of the bias corrections (torch's state["step"]) */
  int64_t skipped_steps;   /* steps skipped for a non-finite norm */
  int64_t clipped_steps;   /* applied steps with coef < 1 */
  float bias_correction1;      /* 1 - beta1^t            (fp64, rounded to fp32 once, as mmt_adamw_step) */
  float bias_correction2_sqrt; /* sqrt(1 - beta2^t)      (likewise) */
  int32_t reserved1[4];
};
int64_t mmt_guard_state_bytes(void);
/* Per-block sums of squares of grads[0 .. n) into the guard state's slots: add == 0 overwrites every slot
 * (the first tensor of a step), add != 0 adds slot-wise (stream order fixes the order of those adds).
 * grads must be 16-byte aligned; n >= 0. */
int mmt_grad_sqsum(void* stream, const float* grads, int64_t n, int32_t add, void* guard);
/* One workgroup: norm = (float)sqrt(sum of the slots in index order), and
 *     coef = min(1, max_norm / (norm + 1e-6))          (torch.nn.utils.clip_grad_norm_, in fp32)
 * or coef = 1 when max_norm <= 0 or max_norm == +inf (no clipping). A NaN norm gives a NaN coef, as in torch.
 * skip_nonfinite != 0 and a non-finite sum (a NaN or an infinity anywhere in the gradients): ok = 0,
 * skipped_steps += 1, applied_steps and the bias corrections stay as they are, so the skipped step does
 * not advance the bias correction and the host need not know that it was skipped. Otherwise ok = 1,
 * applied_steps += 1 (clipped_steps += 1 when coef < 1) and the bias corrections of t = applied_steps are
 * computed on the device. */
int mmt_guard_finalize(void* stream, float max_norm, int32_t skip_nonfinite, float beta1, float beta2, void* guard);
/* mmt_adamw_step on grads * coef with the bias corrections read from the guard header; returns without
 * reading or writing params / exp_avg / exp_avg_sq when the header's ok is 0. With coef == 1 it computes
 * exactly what mmt_adamw_step computes at step = applied_steps. */
int mmt_adamw_step_guarded(mmt_ctx* ctx, void* stream, float* params, const float* grads, float* exp_avg,
                           float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps,
                           float weight_decay, const void* guard);
/* The three calls above return MMT_ERR_INVALID before any launch for a null guard, n < 0, or a tensor or
 * guard pointer that is not 16-byte aligned. */

/* ---- per-tensor statistics of a flat fp32 buffer, and the first-fault record ----
 * One streaming read of x[0 .. n) gives, for every segment of a segment table, the fp64 sum of squares and the
 * largest magnitude of its finite elements, its NaN and Inf counts and the position of its first non-finite
 * element. Asynchronous on `stream`, no device-to-host copy, no sync.
 *
 * Segments: seg_begin is a device array of nseg + 1 ascending offsets; segment s is x[seg_begin[s] ..
 * seg_begin[s + 1]). Offsets need not be multiples of 4 and a segment may be empty. Tensors that are padded
 * apart are described by giving every gap a segment of its own (an unnamed one: the caller ignores its
 * statistics); elements below seg_begin[0] or from seg_begin[nseg] on belong to no segment. What lies in a gap
 * or outside the table influences no other segment's statistics. Offsets are clamped to [0, n] on the device.
 *
 * A record is mmt_stats_record_bytes(nseg) bytes, 16-byte aligned: struct mmt_stats_header at offset 0, then
 * mmt_tensor_stat[nseg]. The scratch is mmt_stats_scratch_bytes(n, nseg) bytes, 16-byte aligned, contents
 * undefined before and after a call (one 32-byte partial per overlapping (chunk of MMT_STATS_CHUNK elements,
 * segment) pair). x must be 16-byte aligned.
 *
 * mode MMT_STATS_ALWAYS: the record is overwritten and valid = 1. `guard` (nullable) is an optimizer's guard
 * state: its applied / skipped counts are copied into the header (0 without one).
 * mode MMT_STATS_ON_SKIP (needs a guard; call it after mmt_guard_finalize and before the guarded steps, the
 * gradients are intact there): the record is written only when the guard header's ok == 0 AND the record's
 * valid == 0; otherwise the launches return after one uniform load each, make no pass over x and leave the
 * record byte for byte as it was. So the first skipped step after arming is kept until the caller re-arms
 * with a 4-byte memset of `valid` to 0 on the same stream.
 *
 * Three launches: per-chunk segmented partials (fp64 from the per-thread accumulator on, fixed trees, plain
 * stores), one wave per segment that adds its chunk partials in a fixed order, and a one-thread commit that
 * alone writes the header. No float atomics, no workgroup waits for another, and no workgroup reads a word
 * another workgroup of the same call writes: the record is bit-identical run to run for identical input.
 * sqsum is within (elements of the segment) * 2^-53 relative of the exact sum (each fp32 square is exact in
 * fp64, all terms are non-negative); the other fields are exact.
 * MMT_ERR_INVALID before any launch for: a null x with n > 0, a null seg_begin / scratch / record, n < 0,
 * nseg < 0, an unknown mode, x / scratch / record not 16-byte aligned, guard not 16-byte aligned, ON_SKIP
 * without a guard. nseg == 0 is valid and writes the header only. */
struct mmt_tensor_stat {      /* 40 bytes, one per segment */
  double sqsum;               /* fp64 sum of x^2 over the FINITE elements of the segment */
  int64_t nan_count;
  int64_t inf_count;          /* +Inf and -Inf */
  int64_t first_bad;          /* index inside the segment of its first non-finite element, -1: none */
  float absmax;               /* max |x| over the finite elements, 0 when there is none */
  float reserved;
};
struct mmt_stats_header {     /* 32 bytes at offset 0 of a stats record; mmt_tensor_stat[nseg] follow */
  int32_t valid;              /* 0: empty / armed, 1: holds a snapshot */
  int32_t nseg;
  int64_t applied_steps;      /* the guard header's counters when the snapshot was taken (0 without a guard) */
  int64_t skipped_steps;
  int64_t reserved;
};
#define MMT_STATS_CHUNK 4096  /* elements per first-pass workgroup */
enum { MMT_STATS_ALWAYS = 0, MMT_STATS_ON_SKIP = 1 };
int64_t mmt_stats_chunk(void); /* MMT_STATS_CHUNK, for callers that cannot read this header */
int64_t mmt_stats_record_bytes(int32_t nseg);           /* -1 for nseg < 0 */
int64_t mmt_stats_scratch_bytes(int64_t n, int32_t nseg); /* -1 for n < 0 or nseg < 0 */
int mmt_tensor_stats(void* stream, const float* x, int64_t n, const int64_t* seg_begin /* device, [nseg + 1] */,
                     int32_t nseg, int32_t mode, const void* guard /* nullable */, void* scratch, void* record);

/* In-place gradient accumulation: with on != 0, stage 0 of mmt_backward / mmt_backward_stage does not zero
 * `grads`, so the backward adds its gradient to what the buffer holds (every writer into `grads` adds:
 * float atomics, the ordered sums, the split-K slab reduce and the one-pass weight-gradient epilogue all
 * read-modify-write). The caller zeroes or overwrites the buffer before the first micro-batch (or runs that
 * one with the switch off). Per context, off by default, read at stage 0: one backward runs under one
 * setting. In deterministic mode the accumulated gradient is still bit-identical run to run. */
int mmt_set_grad_accumulate(mmt_ctx* ctx, int32_t on);
int32_t mmt_get_grad_accumulate(const mmt_ctx* ctx);

/* directional metric for one numeric modality: logits fp32 [batch, T, V]; xb/yb int64 [batch, T];
 * vocab fp64 [V]; accumulates wins_losses[0..1] (int32) and certainty_sum (fp64) on device */
int mmt_eval_direction(mmt_ctx* ctx, void* stream, int32_t batch, int32_t T, int32_t V, const float* logits,
                       const int64_t* xb, const int64_t* yb, const double* vocab, int32_t is_percent,
                       int32_t* wins_losses, double* certainty_sum);

/* live kernel timing (no reference counterpart: the reference has no profiler):
 * HIP events around every engine launch whose label matches one of the comma-separated
 * patterns of `label` — an exact label ("ffn0", "attn_fwd", "attn_bwd", "qkv1_dw", ...), "*suffix"
 * ("*_dw": every weight-gradient GEMM) or "prefix*" — recorded on the stream that launch runs on
 * (the side stream for weight gradients). NULL or "" disables. Each recorded launch carries its
 * algorithmic flops and HBM bytes (every operand read once, every output written once; attention
 * causal-useful). mmt_probe_read_at waits for the events of pattern `pattern` (-1: all) and
 * returns the summed device time, launch count, flops and bytes; mmt_probe_read = all patterns. */
int mmt_probe_set(mmt_ctx* ctx, const char* label);
int32_t mmt_probe_count(const mmt_ctx* ctx);
int mmt_probe_read(mmt_ctx* ctx, double* total_ms, int64_t* launches);
int mmt_probe_read_at(mmt_ctx* ctx, int32_t pattern, double* total_ms, int64_t* launches, double* flops,
                      double* bytes);
/* Pause (on = 0) / resume (on != 0) the probe's recording without clearing it: the bench samples
 * one step in eight, so the probe's event records stay out of the other steps. */
int mmt_probe_enable(mmt_ctx* ctx, int32_t on);
/* Serial mode for measurement: on = 0 runs every launch of this context on the caller's stream (no
 * side stream for the weight gradients and keep bits), on != 0 restores the default. Latched: the
 * next mmt_forward applies it (a forward and its backward always run under one setting). */
int mmt_set_side_stream(mmt_ctx* ctx, int32_t on);

/* Deterministic training mode (the counterpart of torch.use_deterministic_algorithms for this engine's
 * backward): on != 0 makes mmt_backward / mmt_backward_stage write BIT-IDENTICAL gradients whenever the
 * build, the device model, the environment knobs (MMT_* variables and the *_set_* tuning calls), the batch
 * size, the parameters, the inputs and the dropout seed are the same. Every sum that otherwise leaves its
 * kernel as one float atomic per block (bias, LayerNorm weight / bias, per-head stage-2 and embedding-table
 * gradients: added in arrival order, so their low bits change run to run) is instead stored as per-block
 * partials in the workspace and added by one ordered-sum launch in block-index order. The forward, the
 * split-K weight gradients, the loss and AdamW are order-fixed in both modes, so with the mode on a whole
 * training run replays bit for bit. Per context, off by default, and latched like mmt_set_side_stream: the
 * next mmt_forward applies it, a forward and its backward always run under one setting.
 * mmt_workspace_bytes does not depend on the switch (the scratch is always planned).
 * What it does NOT promise: equal bits across different knob settings or builds (they change tile shapes
 * and therefore the partials), across side stream on and off, between this mode and the default mode
 * (same sums, another order: equal to rounding), or for the cross-rank all-reduce of a data-parallel run
 * (world size > 1), which is outside this library.
 * The token-table gradient has a fixed order only through the stable row sort (batch * block_size <= 16384
 * rows, vocabularies <= 16384, n_embd <= 1024): outside that, mmt_backward / stage 0 return
 * MMT_ERR_UNSUPPORTED in this mode before launching anything (the default mode runs as before).
 * The ordered-sum launches carry the probe label "det_sum" (mmt_probe_set). */
int mmt_set_deterministic(mmt_ctx* ctx, int32_t on);
int32_t mmt_get_deterministic(const mmt_ctx* ctx); /* the requested setting (what the next forward latches) */

/* Training objective: torch's F.cross_entropy(weight =, label_smoothing =) extended by a position weight.
 * Modality i has logits x [R, V] (R = batch * block_size; row r sits at position r mod block_size), label
 * smoothing eps, class weights w [V] and position weights u [block_size]:
 *   row_r = (1 - eps) w[t_r] (lse_r - x[r, t_r]) + eps / V * sum_c w[c] (lse_r - x[r, c])
 *   D     = sum_r u_r w[t_r]
 *   loss  = sum_r u_r row_r / D
 * row_r is reduction = "none" of torch; with u == 1 the loss is reduction = "mean" (torch divides by
 * sum_r w[t_r] too). D == 0 gives a non-finite loss, as in torch, and raises the modality's non-finite flag bit.
 * The loss kernel writes the logits' gradient times R, so the backward launches are the plain loss's.
 * `spec` is a host array of one entry per modality (copied); NULL stands for the plain mean CE. The device
 * vectors stay the caller's and must outlive the forwards that use them. Per context; read by the next
 * mmt_forward with targets, in training and in evaluation mode. Entries that are all {0, NULL, NULL} are the
 * plain loss: the same kernels, launches and bits as a context that never had a spec. With class or position
 * weights one more launch (probe label "ce_denom") computes every D in a fixed-order fp64 sum; the loss
 * launch keeps its label "ce_fwd". MMT_ERR_INVALID, with nothing changed, for an eps that is NaN or outside
 * [0, 1). The weights' values (finite, >= 0) are the caller's to check: they live on the device.
 * Under data parallelism and gradient accumulation each rank / micro-batch normalises by its own D. */
typedef struct mmt_loss_spec {
  float label_smoothing;        /* 0 <= eps < 1 */
  const float* class_weight;    /* device fp32 [V_i], finite and >= 0, or NULL: all 1 */
  const float* position_weight; /* device fp32 [block_size], finite and >= 0, or NULL: all 1 */
} mmt_loss_spec;
int mmt_set_loss(mmt_ctx* ctx, const mmt_loss_spec* spec); /* host array [M]; NULL: the plain mean CE */
int mmt_get_loss(const mmt_ctx* ctx, mmt_loss_spec* out);  /* [M] */

/* ---- device-resident batcher: get_batch (training_utils.py:333-384) on HBM token streams ---- */
/* in-place random walk of one int32 training stream (data_utils.py:342-351 as reached through
 * training_utils.py:350-360): x += uniform{0,+-1..+-r} where r < x < V - r */
int mmt_batch_jitter(void* stream, int32_t* data, int64_t n, int32_t rand_size, int32_t vocab_size, uint64_t seed,
                     uint64_t counter);
/* batch start indices uniform over valid positions (generate_batch_starting_indices,
 * training_utils.py:33-181): cum_valid / file_start int64 [nfiles] describe the split */
int mmt_batch_indices(void* stream, int32_t batch, const int64_t* cum_valid, const int64_t* file_start, int32_t nfiles,
                      int32_t first_offset, uint64_t seed, uint64_t counter, int64_t* ix);
/* x[m] = data[m][ix : ix+T], y[m] = data[m][ix+1 : ix+T+1] (int64 [batch, T]); data/x/y are host
 * arrays of nmod device pointers */
int mmt_batch_gather(void* stream, int32_t nmod, const int32_t* const* data, const int64_t* ix, int32_t batch,
                     int32_t T, int64_t* const* x, int64_t* const* y);

/* ---- bit-exact device walk: get_batch's jitter (data_utils.py:342-351 through
 * training_utils.py:350-360) with the reference's own Python `random` stream (MT19937) ----
 * mt_state: device uint32[625] = CPython random.getstate()[1] (624 key words + index).
 * words: device buffer of mmt_exact_words_bytes(nwords) bytes; mmt_exact_gen fills it with the
 * generator's stream from mt_state (one workgroup; nwords >= the draws of one walk). mmt_exact_walk
 * walks data[r] (int32, n[r] elements) for every r with rand_size[r] != 0 (0 = None) in order,
 * each eligible element (r < x < V - r) taking the next accepted draw of random.choice, then moves
 * mt_state past the last word drawn. *status is set to 1 if the words ran out (never, at the
 * sizes mmt_exact_words_bytes is asked for by the Python batcher). scratch: see
 * mmt_exact_walk_scratch_bytes(max n[r], nwords). All asynchronous on `stream`. */
int64_t mmt_exact_words_bytes(int64_t nwords);
int64_t mmt_exact_walk_scratch_bytes(int64_t max_n, int64_t nwords);
int mmt_exact_gen(void* stream, const uint32_t* mt_state, uint32_t* words, int64_t nwords);
int mmt_exact_walk(void* stream, int32_t nmod, int32_t* const* data, const int64_t* n, const int32_t* rand_size,
                   const int32_t* vocab, uint32_t* mt_state, const uint32_t* words, int64_t nwords, void* scratch,
                   int64_t scratch_bytes, int32_t* status);
/* tuning knob: bit 0 / bit 1 = the slice-streamed hs-64 attention dK/dV / dQ pass, bit 2 = dK/dV at 3 waves
 * per SIMD, bit 3 = the slice-streamed hs-64 forward, bit 4 unused, bit 5 = the one-pass hs-64 backward at T <= 512 with one
 * KV stream, bit 6 = the one-pass hs-32 backward at T <= 256, bit 7 = that kernel also for several KV streams
 * (default 79 = 15 | 64; env MMT_ATTN_RING, read when the library loads); returns the old value */
int mmt_attn_set_ring(int v);
/* tuning knob: attention dropout keep-bit tiles made per wave by attn_mask_kernel (1, 2, 4, 8 or 16; 0 = the env
 * MMT_MASK_G, read when the library loads; default 16 at T >= 1024, else 8). The bits do not depend on it. Returns
 * the old value */
int mmt_attn_set_mask_g(int g);
/* tuning knob: 1 = the big GEMM launches with K < 1024 (the d512 FFN / cross-attention K/V products) on a
 * 128 x 256 tile at two workgroups per CU instead of the 256 x 256 ping-pong kernel; 0 (default, env
 * MMT_GEMM_T2) = the ping-pong kernel. Returns the old value */
int mmt_gemm_set_t2(int v);

/* ---- primitive kernels (single problem), for kernel-level parity tests ------------------- */
/* GEMM pipeline variant (tuning knob, process-wide). 128x128 tile: bits 0-3 forward / backward-data,
 * bits 4-7 weight gradients: 0 = K-step 64 x 2 LDS stages, 1 = 32 x 2, 2 = 32 x 3, 3 = 32 x 4,
 * 4 = 64 x 3, 5 = 32 x 3 and 6 = 32 x 2 at 3+ blocks per CU (64-row epilogue passes). 256x256 tile:
 * bits 8-11 (0 = environment / default policy, 1 / 2 / 3 = BK 32 x 4 / x 3 / x 2); bit 16: the 256x256 tile
 * whatever K (M, N >= 256); bit 17: the 256x256 ping-pong kernel wherever it is built (weight gradients and the
 * row-wide LayerNorm-fused launches included), bit 18 (without bit 17): never, the 256x256 ring instead; neither:
 * the environment (MMT_GEMM8, MMT_GEMM8_LN, MMT_GEMM8_DW). Returns -1 for a field out of range. variant < 0:
 * the default policy (128x128: 6 for bf16-output epilogues without an aux operand, else 0; 256x256: 1 for
 * the weight gradients, else BK 64 x 2). */
int mmt_gemm_set_variant(int variant);
/* splits: split-K factor of EPI atomic_f32 launches (<= 0: automatic) */
int mmt_op_gemm(void* stream, int32_t a_kc, int32_t b_kc, int32_t epi, int32_t splits, int32_t M, int32_t N,
                int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb, const float* bias,
                const void* aux, int32_t ldaux, const float* resid, int32_t ldres, float* o32, int32_t ldc,
                void* o16, int32_t ldo16, float alpha);
/* The launch plan of a GEMM batch, from sizes alone: no stream, no device memory, no HIP call, so it runs
 * without a GPU (tests/test_gemm_plan_cpu.py pins the dispatch policy with it). kind: 0 = mmt_op_gemm's launcher
 * (a_kc, b_kc, epi, splits as there), 1 = weight gradient (slab_bytes: slab capacity, 0 = none), 2 = residual +
 * LayerNorm forward, 3 = LayerNorm-backward, 4 = MX-fp8 (epi). count problems of M[g] x N[g] x K[g]; lda / ldb:
 * 0 = K (or M / N for an MN-contiguous operand) padded to 8 elements (fp8: 16); tile_hint / dw_blocks: the
 * engine's per-launch hints (0: none); flags bit 0: the fused Q/K/V stage 2 (hh 16), bit 1: the next LayerNorm's
 * output. Writes 16 ints: status (0 ok, 1 nothing to launch, 2 invalid), family (0 ring, 1 ping-pong, 2 fp8),
 * tile (0 = 128x128, 1 = 128x256, 2 = 256x256, 3 = 128x512), K-step, stages, minimum blocks per CU, SWAP,
 * a_kc, b_kc, epi of the kernel, grid x / y / z, slabs (weight gradients: 1 = split-K slabs + reduce, 0 =
 * accumulate in place), the reduce launch's blocks, the XCD-plane flag. */
int mmt_op_gemm_plan(int32_t kind, int32_t a_kc, int32_t b_kc, int32_t epi, int32_t splits, int32_t count,
                     const int32_t* M, const int32_t* N, const int32_t* K, int32_t lda, int32_t ldb, int32_t tile_hint,
                     int32_t dw_blocks, int64_t slab_bytes, int32_t flags, int32_t* plan);
/* Q/K/V projection of the engine's forward (reference model.py:36-50, every head's key / query /
 * value MLP at once): h1[M, N] = bf16(tanh(A[M, K] B[N, K]^T + bias)) (stage 1, N = 3 H hh) and, fused
 * into the same GEMM's epilogue, stage 2 out[m, blk*2hh + o] = bf16(sum_i w2[blk][o][i] h1[m, blk*hh + i])
 * (w2 fp32 [N/hh][2hh][hh]). hh must be 16 or 32 and the GEMM must run on the 128 x 128 tile (not M,
 * N >= 256 with K >= 1024), else MMT_ERR_UNSUPPORTED (the engine then runs stage 2 as mmt_op_qkv2_fwd's
 * separate kernel); ld_out % 8 == 0, 16-B aligned out. */
int mmt_op_gemm_qkv(void* stream, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B,
                    int32_t ldb, const float* bias, void* h1, int32_t ldh1, const float* w2, int32_t hh, void* out,
                    int32_t ld_out);
/* weight gradient out[M, N] += alpha * A[K, M]^T B[K, N] (A, B bf16, MN-contiguous rows of K):
 * split-K into fp32 slabs in `slab` (device scratch of slab_bytes; NULL/0: one K pass) + a reduce
 * pass, the engine's path for every dW of the backward */
int mmt_op_gemm_wgrad(void* stream, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B,
                      int32_t ldb, float* out, int32_t ldc, float alpha, void* slab, int64_t slab_bytes);
/* attention out-projection as ONE fused launch (the engine's forward path at C = 256 / 512; replaces the
 * pair mmt_op_gemm(bias_tanh_bf16) + mmt_op_gemm(bias_resid_f32), reference model.py:82-92 / 102-117):
 *   h[M, C/2]  = bf16(tanh(x[M, C] W0[C/2, C]^T + b0))      (stored: the backward reads it)
 *   out[M, C]  = resid + keep(m, n) * (h W2[C, C/2]^T + b2)  (fp32; hash dropout of drop_key / drop_thr,
 *                kept values times drop_scale, 0: off), out16 (nullable) its bf16 copy;
 *   lnf_y (nullable) = bf16(LayerNorm(out) * lnf_gamma + lnf_beta), lnf_mean / lnf_rstd its row statistics
 * with h kept in LDS between the products. C must be 256 or 512 (else MMT_ERR_UNSUPPORTED); row strides
 * ldx, ldw0 (W0), ldw2 (W2), ldh (h); out / resid / out16 / lnf_y have stride C. */
int mmt_op_mlp2(void* stream, int32_t M, int32_t C, const void* x, int32_t ldx, const void* w0, int32_t ldw0,
                const float* b0, const void* w2, int32_t ldw2, const float* b2, void* h, int32_t ldh, const float* resid,
                float* out, void* out16, uint32_t drop_key, uint32_t drop_thr, float drop_scale, const float* lnf_gamma,
                const float* lnf_beta, void* lnf_y, float* lnf_mean, float* lnf_rstd);
/* its backward-data pair as ONE launch (the engine's backward path at C = 256 / 512; replaces
 * mmt_op_gemm(dtanh_bf16) + mmt_op_gemm(store_bf16)): dh[M, C/2] = bf16(alpha (dy[M, C] W2[C, C/2]) (1 - h^2))
 * with db0 (nullable) += its fp32 column sums, dx[M, C] = bf16(dh W0[C/2, C]); W2 / W0 are the forward
 * weights as stored ([C][C/2] / [C/2][C], row strides ldw2 / ldw0), h the forward's saved tanh output.
 * db0 sums the fp32 values alpha (dy W2) (1 - h^2) BEFORE their bf16 store, not the stored dh (the unfused pair's
 * dtanh_bf16 epilogue sums the same fp32 values); dx is the product of the STORED bf16 dh. Pinned bit for bit by
 * tests/test_gpu_exact_kernels.py test_mlp2_bwd_exact, on inputs where the two sums differ. */
int mmt_op_mlp2_bwd(void* stream, int32_t M, int32_t C, const void* dy, int32_t lddy, const void* w2, int32_t ldw2,
                    const void* h, int32_t ldh, float alpha, const void* w0, int32_t ldw0, void* dh, int32_t lddh,
                    float* db0, void* dx);
/* the FFN forward as ONE launch (the engine's forward path at C = 256, mmt_set_ffn_fused; replaces the pair
 * mmt_op_gemm(bias_relu_bf16) + mmt_op_gemm(bias_resid_f32) and gives its bits, reference model.py:162-175, 225),
 * for `count` (1..4) problems that share the weights, problem g with M[g] rows:
 *   h[g][M, 4C] = bf16(relu(x[g][M, C] W0[4C, C]^T + b0))        (stored: the backward reads it)
 *   out[g][M, C] = resid[g] + keep(m, n) * (h W2[C, 4C]^T + b2)   (fp32; hash dropout of drop_key / drop_thr,
 *                  kept values times drop_scale, 0: off), out16[g] (array or entries nullable) its bf16 copy;
 *   lnf_y[g] (array nullable) = bf16(LayerNorm(out) * lnf_gamma + lnf_beta), lnf_mean[g] / lnf_rstd[g] its
 *   row statistics (all of lnf_* or none)
 * with h walked through LDS in 128-column chunks and never read back. x, h, resid, out, out16, lnf_y, lnf_mean,
 * lnf_rstd are host arrays of `count` device pointers. C must be 256 (else MMT_ERR_UNSUPPORTED; so are
 * misaligned pointers or strides); row strides ldx, ldw0 (W0), ldw2 (W2), ldh (h); out / resid / out16 /
 * lnf_y have stride C. */
int mmt_op_ffn(void* stream, int32_t count, const int32_t* M, int32_t C, const void* const* x, int32_t ldx,
               const void* w0, int32_t ldw0, const float* b0, const void* w2, int32_t ldw2, const float* b2,
               void* const* h, int32_t ldh, const float* const* resid, float* const* out, void* const* out16,
               uint32_t drop_key, uint32_t drop_thr, float drop_scale, const float* lnf_gamma, const float* lnf_beta,
               void* const* lnf_y, float* const* lnf_mean, float* const* lnf_rstd);
int mmt_op_layernorm_fwd(void* stream, int32_t R, int32_t C, const float* x, const float* gamma, const float* beta,
                         void* y16, float* mean, float* rstd);
int mmt_op_layernorm_bwd(void* stream, int32_t R, int32_t C, const float* x, const float* gamma, const float* mean,
                         const float* rstd, const float* dy, float* dx, void* dx16, float* dgamma, float* dbeta);
/* backward-data GEMM with the LayerNorm backward of its rows fused (the engine's path when C == 256;
 * replaces the pair mmt_op_gemm(EPI store_f32) + mmt_op_layernorm_bwd, model.py:189-190 under
 * autograd): dy = alpha * A[M, K] B[K, N] (A K-contiguous, B MN-contiguous, bf16), never stored;
 * dx[M, N] += rstd * (g dy - mean(g dy) - xhat mean(g dy xhat)) with xhat = (x - mean) * rstd;
 * dx16 (nullable) = bf16(keep(m, n) * dx) with the hash mask of drop_key / drop_thr (0: no mask,
 * kept values times drop_scale) and dsum (nullable) += its column sums; dgamma += colsum(dy xhat),
 * dbeta += colsum(dy). N must be 256 or 512; row strides: A lda, B ldb, x / dx N, dx16 N.
 * MMT_ERR_UNSUPPORTED when the shape does not fit the fused kernel. */
int mmt_op_gemm_ln_bwd(void* stream, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B,
                       int32_t ldb, float alpha, const float* x, const float* gamma, const float* mean,
                       const float* rstd, float* dx, void* dx16, float* dgamma, float* dbeta, float* dsum,
                       uint32_t drop_key, uint32_t drop_thr, float drop_scale);
/* causal attention over nstreams KV streams; layouts as in the engine (row = b*T + t).
 * lse[j] (float [B*H*T] per stream, written by the forward, read by the backward) is in the LOG2
 * domain: lse = log2(sum_k 2^(log2(e) * scale * q.k)) = ln(sum_k e^(scale q.k)) / ln 2, with scale =
 * hs^-0.5 -- a natural-log LSE from another implementation must be divided by ln 2 first. */
int mmt_op_attention_fwd(void* stream, int32_t B, int32_t T, int32_t H, int32_t hs, int32_t nstreams,
                         const void* q, int32_t q_ld, const void* const* k, const void* const* v, int32_t kv_ld,
                         int32_t kv_hstride, void* o, int32_t o_ld, void* const* oj, float* const* lse);
int mmt_op_attention_bwd(void* stream, int32_t B, int32_t T, int32_t H, int32_t hs, int32_t nstreams,
                         const void* q, int32_t q_ld, const void* const* k, const void* const* v, int32_t kv_ld,
                         int32_t kv_hstride, const void* o, int32_t o_ld, const void* const* oj,
                         const float* const* lse, const void* dout, int32_t dout_ld, float* const* dvec, void* dq,
                         int32_t dq_ld, void* const* dk, void* const* dv, int32_t dkv_ld, int32_t dkv_hstride);
/* the same with a caller scratch of fp32 rows [B*T][>= H*hs] (dq32_ld % 4 == 0, 16-B aligned; contents
 * undefined afterwards): the one-pass hs-32 backward (T <= 256) sums dQ over several KV streams there,
 * so cross-attention takes it too (without scratch it takes the two-pass kernels) */
int mmt_op_attention_bwd_ws(void* stream, int32_t B, int32_t T, int32_t H, int32_t hs, int32_t nstreams,
                            const void* q, int32_t q_ld, const void* const* k, const void* const* v, int32_t kv_ld,
                            int32_t kv_hstride, const void* o, int32_t o_ld, const void* const* oj,
                            const float* const* lse, const void* dout, int32_t dout_ld, float* const* dvec, void* dq,
                            int32_t dq_ld, void* const* dk, void* const* dv, int32_t dkv_ld, int32_t dkv_hstride,
                            float* dq32, int32_t dq32_ld);
/* Dropout of the normalised attention probabilities, as the engine's training forward runs it. The keep bits
 * are made once per (key, shape) by mmt_op_attention_mask and read by the forward and the backward:
 * element (query t, key s) of stream j, head slot bh = b*H + h is kept iff the 16-bit half (s & 1) of
 * prob_hash(hash(hash(drop_key, j, stream salt), bh*T + t, row salt), s >> 1) is >= drop_thr (csrc/mmt_common.h;
 * drop_thr = 0: no dropout, nothing read or written); kept probabilities are scaled by drop_scale.
 * mmt_op_attention_mask fills the buffers of `count` (1..8) problems of one shape in one launch: nstreams,
 * drop_key and drop_thr are host arrays of `count` entries, dmask a host array of count * 8 device pointers
 * (problem g, stream j at dmask[g * 8 + j]; entries j >= nstreams[g] are not read), each to
 * mmt_op_attention_mask_dwords(B, H, T) dwords: per 32 x 32 tile (bh, query tile qt, key tile kt <= qt), index
 * bh * ntri + qt (qt + 1) / 2 + kt, a 32-dword key-major record, then after all of those the tiles' 32-dword
 * lane-word records. MMT_ERR_INVALID before any launch for count outside 1..8, a null array, nstreams[g] outside
 * 1..8 or a null buffer of a problem with drop_thr != 0. */
int64_t mmt_op_attention_mask_dwords(int32_t B, int32_t H, int32_t T);
int mmt_op_attention_mask(void* stream, int32_t count, int32_t B, int32_t T, int32_t H, const int32_t* nstreams,
                          const uint32_t* drop_key, const uint32_t* drop_thr, uint32_t* const* dmask);
/* mmt_op_attention_fwd / _bwd_ws with that dropout (dmask: host array of nstreams device pointers, filled by
 * mmt_op_attention_mask for the same drop_key, drop_thr, B, T, H; not read when drop_thr == 0, then the calls
 * are the ones above). MMT_ERR_INVALID for drop_thr != 0 with a null dmask. */
int mmt_op_attention_fwd_drop(void* stream, int32_t B, int32_t T, int32_t H, int32_t hs, int32_t nstreams,
                              const void* q, int32_t q_ld, const void* const* k, const void* const* v, int32_t kv_ld,
                              int32_t kv_hstride, void* o, int32_t o_ld, void* const* oj, float* const* lse,
                              uint32_t drop_key, uint32_t drop_thr, float drop_scale, uint32_t* const* dmask);
int mmt_op_attention_bwd_drop(void* stream, int32_t B, int32_t T, int32_t H, int32_t hs, int32_t nstreams,
                              const void* q, int32_t q_ld, const void* const* k, const void* const* v, int32_t kv_ld,
                              int32_t kv_hstride, const void* o, int32_t o_ld, const void* const* oj,
                              const float* const* lse, const void* dout, int32_t dout_ld, float* const* dvec, void* dq,
                              int32_t dq_ld, void* const* dk, void* const* dv, int32_t dkv_ld, int32_t dkv_hstride,
                              float* dq32, int32_t dq32_ld, uint32_t drop_key, uint32_t drop_thr, float drop_scale,
                              uint32_t* const* dmask);
/* KV-cache decode attention, the kernel under mmt_decode_step: ONE query position t (0 <= t < T) per sequence
 * against the cached keys / values of positions 0..t, one softmax per KV stream (scale = hs^-0.5), the
 * per-stream outputs summed. q and o are compact [B, *] bf16 (row b, head h at column h*hs, row strides q_ld /
 * o_ld); the cache of stream j is k[j] / v[j], bf16 [B*T, kv_ld]: position s of sequence b is row b*T + s, head
 * h at column h*kv_hstride (self-attention: the forward's [B*T, 3C] Q/K/V rows with k = +0, v = +2C, kv_hstride
 * = hs; cross-attention: per-stream [B*T, 2C] rows with v = k + hs, kv_hstride = 2 hs). Rows s > t are never
 * read; only columns [h*hs, (h+1)*hs) of o are written. Arithmetic is fp32 on the bf16 values, o is rounded
 * once. Before any launch: MMT_ERR_INVALID for a null pointer, B or H < 1, nstreams outside 1..8, t outside
 * 0..T-1, or q_ld / kv_ld / kv_hstride not a multiple of 8 (16-byte loads; the pointers must be 16-B aligned
 * too); MMT_ERR_UNSUPPORTED for hs not in {8, 16, 24, 32, 48, 64}. */
int mmt_op_attention_decode(void* stream, int32_t B, int32_t t, int32_t T, int32_t H, int32_t hs, int32_t nstreams,
                            const void* q, int32_t q_ld, const void* const* k, const void* const* v,
                            int32_t kv_ld, int32_t kv_hstride, void* o, int32_t o_ld);
/* Sample fan-out decode attention, the kernel under mmt_decode_fanout_step: q and o are compact [B*samples, *],
 * row r = b*samples + s. Keys / values of positions 0..n0-1 of row r are the cache rows b*T + p of k[j] / v[j] (as
 * above), positions n0..t its own tail rows r*tail_rows + (p - n0) of tail_k[j] / tail_v[j], bf16
 * [B*samples*tail_rows, tail_ld], head h at column h*kv_hstride. One softmax per stream over the t + 1 keys, the
 * outputs summed. A workgroup serves 16 samples of one (prompt, head): a prefix row is fetched once for the 16.
 * Cache rows >= n0, tail rows > t - n0 and rows of samples >= `samples` are never read or written; fp32 scores and
 * probabilities (flash-style running maximum over 64-key tiles), o rounded once; bit-identical run to run, and
 * a sample's output does not depend on the other samples of the launch. Before any launch: the checks of
 * mmt_op_attention_decode, and MMT_ERR_INVALID for samples < 1, n0 outside 1..t, tail_rows <= t - n0, a null
 * tail pointer or tail_ld not a multiple of 8. */
int mmt_op_attention_decode_fanout(void* stream, int32_t B, int32_t samples, int32_t n0, int32_t t, int32_t T,
                                   int32_t H, int32_t hs, int32_t nstreams, const void* q, int32_t q_ld,
                                   const void* const* k, const void* const* v, int32_t kv_ld, int32_t kv_hstride,
                                   const void* const* tail_k, const void* const* tail_v, int32_t tail_ld,
                                   int32_t tail_rows, void* o, int32_t o_ld);
/* Rolling-window fan-out attention, the kernel under mmt_rolling_step: every row r = b*samples + s has m tail
 * positions and all of them are queries, in ONE launch. q and o are compact [B*samples*m, *]: query (r, i) is row
 * r*m + i. Its keys / values are the cache rows b*T + 0..p-1 of k[j] / v[j], then the row's own tail rows r*m + 0..i
 * of tail_k[j] / tail_v[j] (bf16 [B*samples*m, tail_ld]; tail_rows must equal m). The arithmetic of query (r, i) is
 * mmt_op_attention_decode_fanout's at n0 = p, t = p + i on the same buffers with tail_rows = m (one device function
 * serves both kernels): the same bits. Cache rows >= p, tail rows of other samples and rows past B*samples*m are
 * never read or written. Before any launch: the checks of mmt_op_attention_decode_fanout with p for n0 and
 * p + m - 1 for t (so p >= 1, m >= 1, p + m <= T), and MMT_ERR_INVALID for tail_rows != m. */
int mmt_op_attention_rolling_fanout(void* stream, int32_t B, int32_t samples, int32_t p, int32_t m, int32_t T,
                                    int32_t H, int32_t hs, int32_t nstreams, const void* q, int32_t q_ld,
                                    const void* const* k, const void* const* v, int32_t kv_ld, int32_t kv_hstride,
                                    const void* const* tail_k, const void* const* tail_v, int32_t tail_ld,
                                    int32_t tail_rows, void* o, int32_t o_ld);
/* hs-32 causal self-attention (T <= 256) with Q / K / V made on chip: in place of q / k / v the kernels take
 * the stage-1 rows h1 (bf16 [B*T][ld_h1], ld_h1 % 8 == 0, 16-B aligned; column block blk = kind * H + head of
 * 16 columns, kinds K, Q, V; pad columns and rows past the batch are never read) and w2 (fp32 [3 H][32][16],
 * 16-B aligned) and compute X = bf16(h1_blk bf16(W2_blk)^T) per (batch, head) themselves: the same bits as
 * mmt_op_qkv2_fwd's rows. The backward returns the stage-2 gradients: dh1 (bf16, ld_h1; only the 3 H 16 columns
 * are written), dw2 and db1 (fp32 [3 H][32][16] and [3 H * 16], accumulated by atomics). MMT_ERR_UNSUPPORTED
 * when the shape or the alignment does not fit (or mmt_attn_set_ring bit 6 is off, for the backward). */
int mmt_op_attention_fwd_h1(void* stream, int32_t B, int32_t T, int32_t H, const void* h1, int32_t ld_h1,
                            const float* w2, void* o, int32_t o_ld, float* lse);
int mmt_op_attention_bwd_h1(void* stream, int32_t B, int32_t T, int32_t H, const void* h1, int32_t ld_h1,
                            const float* w2, const void* o, int32_t o_ld, const float* lse, const void* dout,
                            int32_t dout_ld, void* dh1, float* dw2, float* db1);
/* the same two with dropout of the probabilities (one stream: dmask is the device buffer itself) */
int mmt_op_attention_fwd_h1_drop(void* stream, int32_t B, int32_t T, int32_t H, const void* h1, int32_t ld_h1,
                                 const float* w2, void* o, int32_t o_ld, float* lse, uint32_t drop_key,
                                 uint32_t drop_thr, float drop_scale, uint32_t* dmask);
int mmt_op_attention_bwd_h1_drop(void* stream, int32_t B, int32_t T, int32_t H, const void* h1, int32_t ld_h1,
                                 const float* w2, const void* o, int32_t o_ld, const float* lse, const void* dout,
                                 int32_t dout_ld, void* dh1, float* dw2, float* db1, uint32_t drop_key,
                                 uint32_t drop_thr, float drop_scale, uint32_t* dmask);
/* The launch plan of an attention batch, from numbers alone: no stream, no device memory, no HIP call, so it runs
 * without a GPU (tests/test_attn_plan_cpu.py pins the dispatch policy with it). pass: 0 forward, 1 backward, 2 the
 * keep-bit mask. count problems of one shape with nstreams[g] KV streams. ld: NULL, or 10 ints of which a 0 means
 * the packed default (C = H * hs): q_ld, kv_ld, kv_hstride (hs), o_ld, dout_ld, dq_ld, dkv_ld, dkv_hstride (hs),
 * dq32_ld, the h1 rows' (3 H * 16). flags: bit g (g < 8) dropout on in problem g; 0x100 the stage-2 fields, 0x200
 * the on-chip Q/K/V fields, 0x400 the fp32 dQ scratch, 0x800 deterministic partials; 0x1000 / 0x2000 / 0x4000 /
 * 0x8000 the Q / dO / dQ / O base at 8 mod 16 bytes; 0x10000 the backward as mmt_backward asks before it sets the
 * stage-2 fields (taken as present and aligned). Writes 32 ints: status (0 ok, 1 nothing to launch, 2 invalid),
 * the number of launches (2: the dQ pass, then dK/dV), then per launch 14 ints, the second launch's 0 when there is
 * one: family (0 chunked forward, 1 chunked dQ, 2 chunked dK/dV, 3 hs-64 ring forward, 4 ring dQ, 5 ring dK/dV,
 * 6 one-pass hs-64 backward, 7 one-pass hs-32 backward, 8 on-chip-QKV hs-32 forward, 9 mask), hs, DROP, the
 * one-pass hs-32 kernel's MS / Q2 / DET / OC, the dK/dV ring's waves per SIMD, ring depth, the mask kernel's tiles
 * per wave, grid x / y / z, workgroup size; last the deterministic launch's floats of partials per problem, a 64-bit
 * count as its low and its high 32 bits. */
int mmt_op_attention_plan(int32_t pass, int32_t count, int32_t B, int32_t T, int32_t H, int32_t hs,
                          const int32_t* nstreams, const int32_t* ld, int32_t flags, int32_t* plan);
int mmt_op_qkv2_fwd(void* stream, int32_t R, int32_t nblk, int32_t hs, const void* h1, int32_t ld_h1,
                    const float* w2, void* out, int32_t ld_out);
int mmt_op_qkv2_bwd(void* stream, int32_t R, int32_t nblk, int32_t hs, const void* h1, int32_t ld_h1,
                    const float* w2, const void* dout, int32_t ld_out, void* dh1, float* dw2);
int mmt_op_colsum(void* stream, int32_t R, int32_t N, const void* x, int32_t ld, float* out, float alpha);
/* the deterministic mode's ordered sum: dst[i] += (((parts[i] + parts[ld + i]) + parts[2 ld + i]) + ...) over
 * nparts partial vectors of n floats (row stride ld >= n), plain fp32 adds in index order (no FMA, no tree) */
int mmt_op_ordered_sum(void* stream, int32_t nparts, int32_t n, const float* parts, int64_t ld, float* dst);
int mmt_op_cross_entropy(void* stream, int32_t R, int32_t V, const float* logits, const int64_t* tgt,
                         void* dlogits, int32_t ld_d, float* loss);
/* the loss kernel of mmt_set_loss on caller buffers (rows at position r mod T): the D pre-pass when class_weight
 * or position_weight is set (then denom, one device double, is required and receives D), then the loss and
 * dlogits = R * dloss / dlogits. loss is accumulated (+=). part: nullable float [512], the block shares summed in
 * block order (run-to-run identical bits); flag: nullable int [2], both words |= 1 for a non-finite loss.
 * MMT_ERR_INVALID for R, T, V < 1, ld_d < V, eps outside [0, 1) and weights without denom. */
int mmt_op_cross_entropy_spec(void* stream, int32_t R, int32_t T, int32_t V, const float* logits, const int64_t* tgt,
                              void* dlogits, int32_t ld_d, float* loss, float eps, const float* class_weight,
                              const float* position_weight, double* denom, float* part, int32_t* flag);
int mmt_op_embedding_fwd(void* stream, int32_t B, int32_t T, int32_t C, int32_t V, const int64_t* idx,
                         const float* tok, const float* pos, float* x);
int mmt_op_embedding_bwd(void* stream, int32_t B, int32_t T, int32_t C, int32_t V, const int64_t* idx,
                         const float* dx, float* dtok, float* dpos);
/* the same with a caller scratch of >= B*T*C floats (the engine passes a free backward buffer): each
 * row chunk's LDS-privatised token-table slabs are stored there and one reduce pass adds them into
 * dtok, so the rows split into short chunks without global atomics; dtok is accumulated (+=) */
int mmt_op_embedding_bwd_ws(void* stream, int32_t B, int32_t T, int32_t C, int32_t V, const int64_t* idx,
                            const float* dx, float* dtok, float* dpos, float* scratch);
// token-table gradient variant of the scratch path (mmt_op_embedding_bwd_ws, the engine's): 1 (default,
// env MMT_EMB_SORT) = counting sort of the rows by token + run sums (no LDS float atomics), 0 = the
// LDS-privatised slabs with per-chunk partial tables; returns the previous value (tests, A/B)
int mmt_emb_set_sort(int on);
// per-head Q/K/V stage-2 backward at hs 32 / 64 (mmt_op_qkv2_bwd, the engine's): bit 0 (hs 32) / bit 1
// (hs 64) set = each load instruction reads whole row slices and the tile is redistributed through
// LDS, clear = loads in the MFMA fragment layout; default 2 (env MMT_QKV2_COAL); returns the previous
// value (tests, A/B)
int mmt_qkv2_set_coal(int on);
// FFN ReLU' as bits (the ffn0 epilogue writes one bit per hidden element, the ffn2 data gradient reads
// them instead of the bf16 hidden rows): 1 = on, 0 = off (default, env MMT_RELU_BITS). Latched by
// mmt_create (the bit rows are part of that context's workspace); returns the previous value (tests, A/B)
int mmt_set_relu_bits(int on);
// the FFN backward's dropout-masked bf16 residual-gradient copy and FFN output-bias gradient: 1 (default,
// env MMT_DROP_COPY_FUSE) = in the epilogue of the last cross-attention K/V data-gradient GEMM that
// accumulates into that residual gradient, 0 = a separate pass; returns the previous value (tests, A/B)
int mmt_set_drop_copy_fuse(int on);
// hs 32 self-attention backward: 1 (default, env MMT_ATTN_QKV2) = the Q/K/V stage-2 backward (dh1 =
// (dX W2) * tanh', dW2, db1) in the one-pass attention backward's epilogue, dQ / dK / dV never written;
// 0 = the separate stage-2 backward over bf16 dQ / dK / dV. Read at every step; returns the previous value
int mmt_set_attn_qkv2(int on);
// hs 32 self-attention, T <= 256, bf16, forwards with training != 0, where mmt_set_attn_qkv2's path runs: the
// attention kernels make Q / K / V themselves from the stage-1 rows h1 and the head's W2 blocks (the same bits
// the stage-1 GEMM's epilogue stores). Bit 0: the forward does; bit 1: the one-pass backward does. With both
// bits (3, default, env MMT_ATTN_QKV_ONCHIP) the GEMM drops its stage-2 epilogue and the Q/K/V rows are never
// written: mmt_decode_step after such a forward fails with MMT_ERR_INVALID (prefill with training = 0). One
// bit alone still writes them (for measuring each kernel's share). Latched by mmt_forward for that forward
// and its backward; returns the previous value (tests, A/B)
int mmt_set_attn_qkv_onchip(int bits);
// rows per workgroup of the fused out-projection MLP forward at C = 256 (mmt_op_mlp2 and the engine's):
// 128 (8 waves, one workgroup per CU) or 64 (4 waves, three per CU); default 128 (env MMT_MLP2_BM);
// returns the previous value (tests, A/B)
int mmt_mlp2_set_bm(int bm);
// the FFN forward at C = 256, bf16, ReLU bits off (training and eval forwards; decode keeps its own GEMMs):
// 1 (default, env MMT_FFN_FUSED) = one launch per layer (ffn_fwd_kernel: the hidden activation walks through
// LDS, is stored for the backward and never read back), 0 = the ffn0 + ffn2 GEMM pair. Both give the same bits
// where ffn2 runs with its fused LayerNorm on the ping-pong kernel (the default). Read at every forward; returns
// the previous value (tests, A/B)
int mmt_set_ffn_fused(int on);

/* ---- MX-fp8 primitives (C4's fp8 path; BASELINE configs[4]) --------------------------------
 * MX-fp8 = OCP e4m3fn bytes + one E8M0 exponent byte (bias 127) per 32 consecutive K elements of a
 * row: exponent e = the smallest with amax(block) / 2^e <= 448, value = fp8(x * 2^-e) (RNE). */
int mmt_op_mx_quant(void* stream, int32_t rows, int32_t cols, const float* src, int32_t ld_src, void* dst8,
                    int32_t ld8, void* s8, int32_t lds8);
/* Y = X W^T on MX-fp8 X [M][K] (lda bytes) / W [N][K] (ldb bytes) with exponents sa [M][lds_a],
 * sb [N][lds_b] (K % 32 == 0, lds % 4 == 0); epi as mmt_op_gemm's forward epilogues; o8 / s8
 * (nullable): an MX-fp8 copy of a bf16 output (N % 32 == 0) */
int mmt_op_gemm_f8(void* stream, int32_t epi, int32_t M, int32_t N, int32_t K, const void* A8, int32_t lda,
                   const void* sa, int32_t lds_a, const void* B8, int32_t ldb, const void* sb, int32_t lds_b,
                   const float* bias, const float* resid, int32_t ldres, float* o32, int32_t ldc, void* o16,
                   int32_t ldo16, void* o8, int32_t ld8, void* s8, int32_t lds8);
/* LayerNorm forward that also writes an MX-fp8 copy of its output (C % 32 == 0) */
int mmt_op_layernorm_fwd_f8(void* stream, int32_t R, int32_t C, const float* x, const float* gamma, const float* beta,
                            void* y16, float* mean, float* rstd, void* y8, int32_t ld8, void* s8, int32_t lds8);

#ifdef __cplusplus
}
#endif
#endif /* MMT_H_ */
