/*
 * mgea.h -- C ABI of the MI355X-native (gfx950) transformer-inference hot path of
 * RohitMurali18/Music-Generation-Emotion-Adaptive.
 *
 * The reference has no FFI / plugin interface: its hot path is reached by plain
 * Python attribute access from api_cache.py.  This header is therefore the boundary a maintainer
 * would bind from Python (ctypes stub in INTEGRATION.md); every entry point names the reference
 * code it replaces.  Conventions:
 *   - plain pointers and sizes only; every `*_dev` pointer is a device (HBM) pointer owned by the
 *     caller (in practice a torch.Tensor's data_ptr()) and only borrowed for the call, except the
 *     weight arena, which must outlive the handle created on it;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued on it, nothing synchronises unless stated;
 *   - every function returns 0 on success or a negative MGEA_E* code; mgea_last_error() gives
 *     the thread-local message.  No exception crosses this boundary;
 *   - handles are internally locked: concurrent calls on one handle serialise (the reference's
 *     endpoint runs in FastAPI's thread pool, api_cache.py:186-187).
 */
#ifndef MGEA_H
#define MGEA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGEA_OK          0
#define MGEA_EINVAL     -1   /* bad shape / argument (python: ValueError / RuntimeError) */
#define MGEA_ENOMEM     -2   /* device allocation failed */
#define MGEA_EHIP       -3   /* a HIP call failed */
#define MGEA_ECAPACITY  -4   /* batch or context exceeds what the handle reserved */
#define MGEA_ENODEVICE  -5   /* no gfx950 device visible */

/* Storage / arithmetic modes.  Which engine accepts which:
 *   decoder (mgea_decoder_config.dtype): F32, F16        DistilBERT (mgea_bert_config.dtype): F32, BF16
 * F32 is the parity mode of both (bit-exact greedy ids / labels against the reference's fp32 CPU path). */
#define MGEA_DTYPE_F32   0   /* parity mode: fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) */
#define MGEA_DTYPE_BF16  1   /* DistilBERT perf mode: bf16 weights + activations, fp32 accumulate (bf16 MFMA); calls of fewer than 512
                                tokens (one text per request) run on the exact-fp32 kernels of the same engine */
#define MGEA_DTYPE_F16   2   /* decoder perf mode: fp16 projection matrices + fp16 KV pages, fp32 accumulate (f16 MFMA).  DECODE steps and
                                prefills of up to 512 (row, token) pairs keep the residual stream, LayerNorm, softmax and logits in fp32.
                                A BIG prefill into an empty cache (>= 256 tiles of 256 x 256: e.g. [64, 1024]; switch decoder_prefill16)
                                runs on the f16 matrix cores with fp16 activations between the GEMMs -- the residual stream too, saturated
                                at +-65504 where it is written; accumulation, LayerNorm statistics, softmax and logits stay fp32.  Checked
                                against the oracle on synthetic weights only (tests/test_gpu_f16.py); a trained checkpoint whose residual
                                stream leaves the fp16 range would be clipped there: parity on trained weights is unpinned. */

#define MGEA_BLOCK_PRELN_GELU  0  /* api_cache.py:51-74 GPTBlock (KV-cache model, the default) */
#define MGEA_BLOCK_POSTLN_RELU 1  /* generate_music/generate.py:25-35 nn.TransformerEncoder twin */

#define MGEA_POS_REFERENCE 0 /* pos_emb[:T] per call: every decode step uses row 0 (api_cache.py:99) */
#define MGEA_POS_ABSOLUTE  1 /* true positions (build-defined extra, parity unpinned) */
#define MGEA_POS_CAUSAL    2 /* a standard causal GPT: true positions, a causal mask, every token fed once.  MGEA_BLOCK_PRELN_GELU only.
                                - position of a token = its index in the row; positions past the table clamp to its last row, as
                                  MGEA_POS_ABSOLUTE does;
                                - mgea_decoder_forward appends all T tokens, token t attending the cache and the new tokens <= t, and
                                  returns their causal logits; forward(a) then forward(b) is forward(a | b);
                                - mgea_decoder_step feeds what it is given at position ctx_len (T == 1: the kernels of every other mode);
                                - the generate calls prefill the prompt WITHOUT its last token (a prompt of one token prefills nothing)
                                  and the first step feeds that token at position len - 1, so after n steps a row's context is
                                  len - 1 + n.  The budget and capacity checks are those of the other modes (Tp + n_steps against
                                  max_ctx): one slot per row conservative here;
                                - mgea_decoder_generate_rows_scheduled (and a schedule given to the calls that extend it) is refused with
                                  MGEA_EINVAL, as are mgea_decoder_set_window and the qkv0 table, which need MGEA_POS_REFERENCE;
                                - MGEA_DTYPE_F16: every prefill runs on the fp32-activation path with fp16 pages; the 16-bit flash
                                  prefill has no causal form, so mgea_decoder_stats out[5] stays 0. */

#define MGEA_KV_PAGE_TOKENS 64 /* tokens per KV page (one wave64 tile) */

const char* mgea_last_error(void);
int mgea_version(void);
/* A/B and test switches (tools/README.md lists them).  The table is filled once, when the library is loaded, from the
 * MGEA_<NAME> environment variables; these two calls read / change an entry at run time.  Nothing on a launch path reads the
 * environment, and no switch is needed in production. */
int mgea_tune_set(const char* name, int32_t value);
int mgea_tune_get(const char* name, int32_t* value_out);
/* number of visible HIP devices, or a negative error */
int mgea_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Decoder: replaces GPTBlock / GPTWithKV / sample_kvcache (api_cache.py:39-106, 159-184).
 * ------------------------------------------------------------------------------------------ */
typedef struct mgea_decoder mgea_decoder;

typedef struct mgea_decoder_config {
    int32_t vocab;      /* len(tok2id), <= 14336 (sampler limit) api_cache.py:109 */
    int32_t seq_len;    /* rows of the position table         api_cache.py:36  */
    int32_t d_model;    /*                                    api_cache.py:37  */
    int32_t n_head;     /* reference hard-codes 8             api_cache.py:112 */
    int32_t n_layer;    /*                                    api_cache.py:31-32 */
    int32_t d_ff;       /* 4*d_model in the reference         api_cache.py:83  */
    int32_t max_batch;  /* rows the KV pool is reserved for */
    int32_t max_ctx;    /* tokens per row the KV pool is reserved for (may exceed seq_len: decode
                           steps use position row 0, so the cache can outgrow the table) */
    int32_t dtype;      /* MGEA_DTYPE_* */
    int32_t block_mode; /* MGEA_BLOCK_* */
    int32_t pos_mode;   /* MGEA_POS_* */
    float   ln_eps;     /* 1e-5 (nn.LayerNorm default) */
} mgea_decoder_config;

/* Sampler: replaces api_cache.py:169-178.  top_k == 1 is the greedy path (exact argmax, ties to
 * the lowest id); otherwise softmax(logits/temperature + (-1e10 outside top-k)) -- exactly top_k
 * entries survive like topk + scatter_ (api_cache.py:172-175), equal logits at the boundary by lowest id -- optionally cut
 * to the top_p nucleus, then one multinomial draw per row from a Philox4x32-10 stream keyed by
 * (seed, row, step) -- matches torch.multinomial in distribution only.
 * The selection, over x = logits / temperature (one fp32 division per entry):
 *   top-k (0 < top_k < vocab, otherwise off): every entry greater than the top_k-th largest is kept, then the entries EQUAL to it by
 *     ascending id until exactly top_k are kept -- ties go to the lowest ids.  -inf is an ordinary value: with fewer than top_k
 *     finite entries, -inf entries are among the kept, with probability exactly 0.
 *   top-p (0 < top_p < 1, otherwise off), over what top-k kept: keep {x >= boundary}, the boundary being the largest x at which the
 *     mass of {x >= boundary} reaches top_p (a mass equal to top_p has reached it) -- an entry is kept iff the mass of the strictly
 *     larger entries is below top_p.  Equal entries are kept or dropped whole, and at least one id is kept.  The masses are the fp32
 *     softmax of the kept entries floored to 2^-40, summed as integers, so the boundary does not depend on the order of summation;
 *     against exact arithmetic it may move by entries whose cumulative mass lies within 2e-5 of top_p.
 *   +0.0 ranks above -0.0 (the order is that of the entries' order-preserving integer keys). */
typedef struct mgea_sampler_config {
    float    temperature;  /* > 0 */
    int32_t  top_k;        /* 0 = no top-k cut */
    float    top_p;        /* <= 0 or >= 1 = no nucleus cut (build-defined; not in the reference) */
    int32_t  eos_id;       /* -1 = none; a row that draws eos_id stops (api_cache.py:181) */
    uint64_t seed;
} mgea_sampler_config;

/* Weight arena: ONE contiguous fp32 device buffer holding every tensor (one RCCL broadcast moves
 * it).  Canonical tensor order, each tensor 256-byte aligned, torch layouts ([out, in] Linear):
 *   0 tok_emb [V,C]   1 pos_emb [L,C]
 *   per layer i (12 tensors, base 2+12*i): ln1_w ln1_b in_proj_w[3C,C] in_proj_b[3C]
 *       out_proj_w[C,C] out_proj_b ln2_w ln2_b fc1_w[F,C] fc1_b fc2_w[C,F] fc2_b
 *   then head_w [V,C], head_b [V].
 * (names after remap_state_dict, api_cache.py:118-134) */
int mgea_decoder_arena_layout(const mgea_decoder_config* cfg, int64_t* offsets_floats /* [n] or NULL */,
                              int32_t* n_tensors, int64_t* total_floats);

int mgea_decoder_create(const mgea_decoder_config* cfg, const float* arena_dev, mgea_decoder** out);
int mgea_decoder_destroy(mgea_decoder* h);
/* create() derives a decode-layout copy of the projection matrices from the arena.  If the caller
 * rewrites the arena afterwards (new checkpoint into the same tensor), call this before the next step. */
int mgea_decoder_refresh_weights(mgea_decoder* h, void* stream);

/* Forget all cached tokens and reserve KV pages for `batch` rows of up to `max_len` tokens. */
int mgea_decoder_reset(mgea_decoder* h, int32_t batch, int32_t max_len, void* stream);

/* model(idx, past_kv) (api_cache.py:87-106): append T new tokens per row to the cache and run the
 * NL blocks with every new token attending to the whole cache, no mask.  ids_dev [B,T] int32;
 * lens_dev [B] int32 or NULL (ragged rows: only the first lens[b] tokens of row b are real; the
 * rest are ignored and never cached, so each row equals its solo run).  logits_out_dev [B,T,V]
 * fp32 or NULL (the sampler's prefill discards them, api_cache.py:163): without a logits buffer nothing reads the last block's
 * output, and the call ends once that block's K | V are in the cache (switch decoder_prefill_full = 1 runs the whole block). */
int mgea_decoder_forward(mgea_decoder* h, const int32_t* ids_dev, const int32_t* lens_dev,
                         int32_t B, int32_t T, float* logits_out_dev, void* stream);

/* One decode step of the sampling loop (api_cache.py:167-179): feed ids_in_dev [B] (NULL = the
 * ids the previous step/generate produced), sample, write ids_out_dev [B] (NULL allowed) and
 * optionally the pre-temperature logits [B,V]. */
int mgea_decoder_step(mgea_decoder* h, const int32_t* ids_in_dev, const mgea_sampler_config* s,
                      int32_t* ids_out_dev, float* logits_out_dev, void* stream);

/* sample_kvcache (api_cache.py:159-184) for a batch: reset, prefill (logits dropped), then
 * n_steps decode steps, the first of which re-feeds each row's last prompt token.  The step is
 * captured once per (batch size, greedy | sampled) into a hipGraph and replayed; the sampler's
 * scalars (seed, temperature, top_k, top_p, eos_id) live in device memory, so a new request with
 * other values reuses the graph (mgea_decoder_stats counts instantiations).  ids_out_dev
 * [B, n_steps] int32; entries after a row's EOS are -1.  Host-synchronises only if eos_id >= 0
 * (to stop early once all rows ended).  Row b draws from Philox stream b under key seed
 * (mgea_row_sampler: this is mgea_decoder_generate_rows with stream_b = b and no budget). */
int mgea_decoder_generate(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev,
                          int32_t B, int32_t Tp, int32_t n_steps, const mgea_sampler_config* s,
                          int32_t* ids_out_dev, void* stream);

/* mgea_decoder_generate with a repetition penalty (HF RepetitionPenaltyLogitsProcessor; the paper's decoding setting is top_p 0.92
 * with penalty 1.1).  At every decode step of row b, seen_b = the SET of row b's real prompt tokens (padding of a ragged prompt
 * excluded) and of the ids the row generated so far; the raw head logit x of every id in seen_b becomes x < 0 ? x * p : x / p (one
 * correctly rounded fp32 operation, p as fp32), unseen ids are untouched, and the sampler then runs unchanged on the result:
 * / temperature, top-k, top-p, softmax, Philox draw.  top_k == 1 is the argmax of the penalized row (ties to the lowest id).  A row
 * that drew eos_id is finished and its set is no longer updated.  The penalty travels in the device record with the other sampler
 * scalars, so one captured graph per (batch size, greedy | sampled) serves every penalty value.  repetition_penalty must be finite
 * and > 0 (MGEA_EINVAL otherwise); < 1 favours repeats; == 1 IS mgea_decoder_generate (same launches, same results). */
int mgea_decoder_generate_penalized(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev,
                                    int32_t B, int32_t Tp, int32_t n_steps, const mgea_sampler_config* s,
                                    float repetition_penalty, int32_t* ids_out_dev, void* stream);

/* Per-row sampler settings (mgea_decoder_generate_rows, mgea_op_sample_rows): one record per batch row.
 *   temperature > 0 and finite; 0 <= top_k <= vocab (0 = no cut, 1 = greedy); top_p as in mgea_sampler_config;
 *   repetition_penalty finite and > 0 (1 = none); eos_id -1 = none;
 *   max_new_tokens: the row's step budget, 0 <= max_new_tokens <= n_steps (0 = n_steps): the row finishes after that many ids;
 *   seed, stream: the row's Philox4x32-10 stream.  Row b draws its step-t number from counter {stream, t, 0, const} under key seed:
 *     counter words {stream, low 32 bits of t, bits 32..63 of t, const} with const = 0x6d676561 (a generation's t is an int32 that
 *     starts at 0, so word 2 is 0 there; the mgea_op_sample* calls take a 64-bit step), key words (low 32 bits of seed, high 32 bits
 *     of seed), and u = (word 0 of the output >> 8) * 2^-24, a multiple of 2^-24 in [0, 1).  The row takes the id whose interval of
 *     the cumulative distribution over the kept ids holds u.  The ORDER in which that cumulative sum runs over the ids is unspecified
 *     (any fixed order gives the same distribution); only the distribution is promised, not the id a given u selects.
 * mgea_decoder_generate is the special case seed_b = seed, stream_b = b, no budget, the same settings on every row.  A row's ids
 * therefore depend on its own record, its prompt and on B (the batch size picks the GEMM / attention forms, whose sums run in other
 * orders) -- not on its index in the batch, nor on the other rows' records: the same (prompt, record) at rows 0 and 5 of a batch of B
 * gives the same ids. */
typedef struct mgea_row_sampler {
    float    temperature;
    int32_t  top_k;
    float    top_p;
    float    repetition_penalty;
    int32_t  eos_id;
    int32_t  max_new_tokens;   /* 0 = n_steps */
    uint64_t seed;
    uint32_t stream;
    uint32_t reserved;         /* 0 */
} mgea_row_sampler;

/* mgea_decoder_generate with one sampler record per row, rows [B] (host memory, read before the call returns): concurrent requests
 * with different settings, seeds and budgets in one batch.  ids_out_dev [B, n_steps] int32; entries after a row's EOS or budget are -1.
 * A row with top_k == 1 takes the exact argmax of its (penalized) logits row, ties to the lowest id, without the temperature division.
 * The step graphs are those of mgea_decoder_generate: the greedy form if every row is top_k == 1 without a penalty, the penalized form
 * (presence bitmaps for every row, mgea_decoder_presence) if any row's penalty is not 1, the sampled form otherwise -- a mixed batch
 * replays what a uniform batch of that size captured.  The call stops early (host poll every 16 steps) once every row has finished.
 * Context: each row needs lens[b] + its budget <= max_ctx; the call reserves min(Tp + n_steps, max_ctx) tokens per row and needs
 * Tp < max_ctx and n_steps <= max_ctx -- a row that would run past the reservation finishes there.  Bad records: MGEA_EINVAL naming
 * the row. */
int mgea_decoder_generate_rows(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                               int32_t n_steps, const mgea_row_sampler* rows, int32_t* ids_out_dev, void* stream);

/* Per-row logit bias and minimum length (mgea_decoder_generate_rows_biased, mgea_op_sample_rows_biased): one record per batch row,
 * next to the row's mgea_row_sampler.  Build-defined (the reference has no logits processors); the HuggingFace equivalents are
 * sequence_bias / suppress_tokens / min_new_tokens, OpenAI's is logit_bias.  At every decode step of row b, on the raw head logits x:
 *   1. the repetition penalty over seen_b, exactly as in mgea_decoder_generate_penalized;
 *   2. x[i] += bias_dev[i], one fp32 add (-inf bans id i); a row with bias_dev == NULL is not touched (no + 0);
 *   3. the token grammar, for a row that has a state (mgea_decoder_set_grammar): x[i] = -inf wherever next[s_b][class_of[i]] < 0;
 *   4. if the row's eos_id >= 0 and it has produced fewer than min_new_tokens ids so far (its step index, word 1 of its Philox
 *      counter), x[eos_id] = -inf;
 *   5. the sampler runs unchanged on the result: / temperature, top-k, top-p, softmax, Philox draw.  top_k == 1 is the exact argmax
 *      of the processed row (ties to the lowest id, no temperature division).  A banned id has probability exactly 0 and is never
 *      drawn, also where it is among the top_k kept because fewer than top_k ids are admissible.
 * Checked on the host (MGEA_EINVAL naming the row): reserved == 0 and 0 <= min_new_tokens <= n_steps.  The caller guarantees the rest,
 * as for cu_seqlens: bias_dev holds vocab fp32 values in device memory, none of them NaN or +inf, at least one finite -- and at least
 * one finite besides eos_id if min_new_tokens > 0 and eos_id >= 0.  A row with no admissible id neither hangs nor faults; it yields
 * id 0. */
typedef struct mgea_row_logits {
    const float* bias_dev;         /* [vocab] fp32 device, NULL = none; rows may share one vector */
    int32_t      min_new_tokens;   /* 0 = none */
    int32_t      reserved;         /* 0 */
} mgea_row_logits;

/* mgea_decoder_generate_rows with one mgea_row_logits per row, logits_rows [B] (host memory, read before the call returns);
 * logits_rows == NULL is exactly mgea_decoder_generate_rows.  The engine copies each row's vector into its own [max_batch][vocab]
 * buffer in stream order (no host sync: the caller's vectors must stay valid until `stream` has passed the call), so the step graphs
 * hold stable pointers and a request with other bias values replays the cached graph.  If any row has a bias or min_new_tokens > 0
 * the generation takes the biased form: the logits-row + sampler sequence of the penalized form with the bias applied in the
 * sampler's registers, presence bitmaps for every row (a penalty of 1 changes nothing), its own step graphs.  Rows without a bias
 * keep the ids they get in a batch of that size in which no row has one.  Otherwise the forms of mgea_decoder_generate_rows are
 * untouched.  mgea_decoder_stats out[7] counts the biased steps. */
int mgea_decoder_generate_rows_biased(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      int32_t* ids_out_dev, void* stream);

/* mgea_decoder_generate_rows_biased that also says how likely each id was, and may be told ids to take.  Build-defined: the reference
 * returns no scores (the serving APIs' counterparts are OpenAI's logprobs, HuggingFace's output_scores / compute_transition_scores).
 * At every decode step of row b, on the raw head logits x of the row:
 *   0. the raw statistics m = max_i x_i and log sum_i exp(x_i - m), fp32, in a fixed order (deterministic from run to run).  In a
 *      guided generation (mgea_decoder_generate_rows_guided) the row of a pair is the guided row g by now: guidance comes before
 *      everything here, and the scored outputs of a guided row are taken over g;
 *   1.-5. the processing steps of mgea_row_logits: penalty, bias, (grammar,) EOS ban, then / temperature, top-k, top-p, softmax,
 *      Philox draw;
 *   6. f = forced_ids_dev[b * n_steps + t] for the row's step index t (word 1 of its Philox counter): f >= 0 replaces the drawn id
 *      for everything downstream -- ids_out, EOS and budget bookkeeping, the presence bitmap, the next step's input; -1 leaves the
 *      draw alone (so does every other negative value).  f >= vocab is clamped to vocab - 1 and sets bit 0 of the sticky error
 *      flags (mgea_decoder_error_flags);
 *   7. with id = what the step writes to ids_out:
 *        logprobs_out[b, t]        = x_id - m - log sum_i exp(x_i - m), natural log, taken over the RAW logits of step 0 -- before
 *                                    penalty, bias, EOS ban, temperature, top-k and top-p: a function of the model alone;
 *        choice_logprobs_out[b, t] = log(e_id / total) under the distribution of step 5, the one the draw was made from: -inf for
 *                                    an id outside the kept set (only a forced id can be), 0 for a greedy row that keeps its argmax.
 *      A finished row (ids_out -1) has 0.0 in both, as have the steps that never ran.
 * forced_ids_dev [B, n_steps] int32 (device) or NULL = nothing forced; it is copied into the engine's own buffer in stream order, so
 * a request with other forced ids replays the cached graph.  choice_logprobs_out_dev may be NULL.  Scoring needs the logits row, so
 * a scored generation never takes the greedy form: all-greedy rows run as top_k == 1 records of the sampled form (the exact argmax,
 * ties to the lowest id -- the ids of mgea_decoder_generate_rows).  "Scored" is part of the step-graph key: unscored calls capture
 * and replay what they always did.  mgea_decoder_stats out[3] counts the scored steps.  Scoring a given continuation under the
 * model is this call with every step forced (the distribution sample_kvcache draws from exists only inside the step loop: the
 * prefill is bidirectional, steps add pos_emb[0], the first step re-feeds the last prompt token). */
int mgea_decoder_generate_rows_scored(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows,
                                      const int32_t* forced_ids_dev, int32_t* ids_out_dev, float* logprobs_out_dev,
                                      float* choice_logprobs_out_dev, void* stream);

/* Token grammars: a finite automaton over token classes, applied as a mask in the sampler and advanced on the device inside the step
 * (guided decoding; build-defined, the reference has none).  A grammar is two tables,
 *   class_of [vocab]           int32: the class 0 <= c < n_class of every id;
 *   next     [n_state][n_class] int32: the state after drawing an id of class c in state s, -1 = ids of that class are banned in s.
 * An engine holds one grammar at a time, shared by all rows (several rule sets: one table with disjoint state ranges); every row of a
 * generation has a start state, -1 = the row is not constrained.  Caps: n_class <= 4096, n_state <= 4096, n_state * n_class <= 1 << 20.
 * The grammar is step 3 of the per-step order of mgea_row_logits: 1. repetition penalty; 2. bias; 3. x[i] = -inf wherever
 * next[s_b][class_of[i]] < 0, s_b = the row's current state; 4. the EOS ban of min_new_tokens; 5. the sampler as it is.  After the
 * step, with id = what the step writes to ids_out (the draw, or a forced id), a row that is not finished moves to
 * next[s_b][class_of[id]].  A negative transition (only a forced id can cause one) leaves the state where it is and sets bit 1 of the
 * sticky error flags (mgea_decoder_error_flags); that id's choice log-probability is -inf.  A row whose mask, bias and EOS ban
 * together leave nothing yields id 0, as a row whose bias bans everything does.  Finished rows and rows with state -1 are not
 * touched: no masking, no + 0.
 *
 * mgea_decoder_set_grammar: host tables, validated on the host before anything is enqueued (MGEA_EINVAL naming the offender): the
 * caps, every class_of value in [0, n_class), every next value in [-1, n_state), every state admits at least one class that has at
 * least one id.  The tables are copied in stream order into buffers the handle owns (allocated at create, so the step graphs hold
 * stable pointers), the call synchronises `stream` before it returns.  n_state == 0 clears the grammar (the tables may be NULL). */
int mgea_decoder_set_grammar(mgea_decoder* h, const int32_t* class_of_host, const int32_t* next_host, int32_t n_state, int32_t n_class,
                             void* stream);
/* mgea_decoder_generate_rows_biased / _scored under the grammar: start_states [B] (host, read before the call returns), -1 = none.
 * With every start state -1, or start_states == NULL, this IS mgea_decoder_generate_rows_biased (logprobs_out_dev == NULL: then
 * forced_ids_dev and choice_logprobs_out_dev must be NULL too) or mgea_decoder_generate_rows_scored: the same launches and ids.
 * Otherwise MGEA_EINVAL if no grammar is set or a start state is >= n_state, and the generation takes the grammar form: the biased
 * form's launch sequence with the grammar sampler (presence bitmaps kept), its own step graphs.  Rows with state -1 keep the ids they
 * have in a batch of that size without a grammar. */
int mgea_decoder_generate_rows_grammar(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                       int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows /* NULL ok */,
                                       const int32_t* start_states /* host [B], -1 = none; NULL ok */,
                                       const int32_t* forced_ids_dev /* NULL ok */, int32_t* ids_out_dev,
                                       float* logprobs_out_dev /* NULL = unscored */, float* choice_logprobs_out_dev /* NULL ok */,
                                       void* stream);
/* Every row's state after the last grammar generation -> out_dev [B] int32 (device); -1 for a row without one. */
int mgea_decoder_grammar_states(mgea_decoder* h, int32_t* out_dev, void* stream);
/* out[0] n_state and [1] n_class of the grammar set now (0: none), [2] mgea_decoder_set_grammar uploads over the handle's lifetime,
 * [3] decode steps of the last generate() that ran in the grammar form (0 if it did not). */
int mgea_decoder_grammar_info(mgea_decoder* h, int64_t* out /* [4] */);

/* Classifier-free guidance between paired rows (build-defined, the reference has none; HuggingFace's counterpart is guidance_scale /
 * UnbatchedClassifierFreeGuidanceLogitsProcessor).  A CONDITIONAL row c names a SHADOW row u = shadow_row: the same generation from
 * a prompt without the conditioning tokens.  At every decode step, on the raw head logits of the two rows,
 *   0. (guidance) g = scale * log_softmax(x_c) + (1 - scale) * log_softmax(x_u), fp32, each row's maximum and log-sum-exp reduced in
 *      a fixed order (deterministic from run to run); g replaces BOTH rows' logits;
 *   1.-5. the per-step order of mgea_row_logits runs on g: penalty, bias, grammar, EOS ban, then / temperature, top-k, top-p, softmax,
 *      Philox draw -- guidance comes before the penalty, as in HuggingFace;
 *   6.-7. forced ids and the scored outputs as in mgea_decoder_generate_rows_scored, with x := g: logprobs_out of a guided row is
 *      log_softmax(g) at the id -- the guided distribution, renormalised --, no longer a function of one prompt alone.
 * One id is drawn per pair and fed to both rows.  There is no hand-off between the rows: before the first step the engine overwrites
 * the shadow row's sampler record (seed, Philox stream and budget included), bias vector, grammar start state, forced ids and --
 * after the prompts have seeded them -- presence bitmap with the conditional row's, so both rows' samplers compute the same function
 * of identical inputs.  A pair's repetition-penalty set is therefore the CONDITIONAL prompt plus the generated ids, and what the
 * caller passes in the shadow row's own records is validated and then ignored.  Everything else stays the row's own: its prompt, KV
 * pages, ctx_len and window evictions.  scale == 1 still mixes (the result is log_softmax(x_c)); scale > 1 extrapolates away from the
 * shadow; scale == 0 is the shadow's distribution. */
typedef struct mgea_row_guidance {
    int32_t shadow_row;   /* the row's shadow row in [0, B), or -1 = the row is not conditional */
    float   scale;        /* finite, >= 0; read only where shadow_row >= 0 */
} mgea_row_guidance;

/* mgea_decoder_generate_rows_grammar with one mgea_row_guidance per row, guide [B] (host memory, read before the call returns).
 * guide == NULL, or every shadow_row == -1, IS mgea_decoder_generate_rows_grammar: the same launches and the same ids.  Checked on
 * the host before anything is enqueued (MGEA_EINVAL naming the row): shadow_row in [-1, B) and not the row itself; a shadow row is
 * not conditional itself; no row is the shadow of two rows; a conditional row's scale is finite and >= 0.  Otherwise the generation
 * is guided: every step is the unguided launch sequence with ONE more launch, the mix, between the head GEMM and the sampler;
 * "guided" is part of the step-graph key (unguided calls capture and replay what they always did), and the pairs and scales live in
 * device vectors the handle owns, so a request with other pairs or scales replays the cached graphs.  A guided generation never
 * takes the greedy form: all-greedy rows run as top_k == 1 records of the sampled form.  ids_out_dev holds every row; a shadow row's
 * line equals its conditional row's.  Rows outside every pair keep the ids they get in an unguided batch of that size and form.
 * A guided call that would be capped -- Tp + n_steps > max_ctx without a KV window -- is refused with MGEA_ECAPACITY: the rows of a
 * pair would be stopped after different numbers of steps.  Under a window nothing is capped and each row evicts on its own schedule. */
int mgea_decoder_generate_rows_guided(mgea_decoder* h, const int32_t* prompt_ids_dev, const int32_t* lens_dev, int32_t B, int32_t Tp,
                                      int32_t n_steps, const mgea_row_sampler* rows, const mgea_row_logits* logits_rows /* NULL ok */,
                                      const int32_t* start_states /* host [B], -1 = none; NULL ok */,
                                      const mgea_row_guidance* guide /* host [B]; NULL ok */,
                                      const int32_t* forced_ids_dev /* NULL ok */, int32_t* ids_out_dev,
                                      float* logprobs_out_dev /* NULL = unscored */, float* choice_logprobs_out_dev /* NULL ok */,
                                      void* stream);
/* out[0] the guidance pairs and [1] the guided decode steps of the last generation (both 0 if it was not guided). */
int mgea_decoder_guidance_info(mgea_decoder* h, int64_t* out /* [2] */);

/* Emotion transitions: a row's prompt K | V swapped in the middle of a generation (build-defined; the reference labels a text's
 * sentences in analyze_emotion_transitions and has nothing downstream that uses them).  The emotion reaches the decoder only through
 * the prompt's [BPM] and [KEY_SIGNATURE] tokens; decode steps use position row 0 and the attention is mask-free over the cache, so
 * "the model now sees prompt B instead of prompt A" is exactly "the K | V of cache positions [0, len_b) of every layer are those a
 * prefill of B caches".
 * A SCHEDULED row has n_segments prompt variants, 1 .. MGEA_SCHEDULE_MAX_SEGMENTS (1 = a plain row), all of the row's prompt length
 * len_b = lens[b].  The call has one lens vector and prompt ids [n_seg_max][B][Tp] with Tp <= 64, so the variants lie in the row's
 * logical page 0; a row with fewer segments than n_seg_max repeats its last variant in the matrix (its later variants are prefilled
 * and never used).  Every row starts in segment 0.  The rule runs at the START of every decode step, for a row that is not finished:
 *   k   = key == 0 ? the row's step index (0 at its first decode step) : its grammar state (the start state at its first step);
 *   seg = #{ s in [0, n_segments - 1) : threshold[s] <= k };
 *   if seg != cur_seg[b]: the K | V of positions [0, len_b) in every layer of the row's pages become the K | V that a prefill of
 *   variant seg caches -- the prefill of the B variant-seg prompts with this call's B, Tp and lens --, bit for bit in the page's
 *   element type; then cur_seg[b] = seg.
 * Nothing else changes: not positions >= len_b (the re-fed duplicate of the last prompt token included), not ctx_len, cur_ids, the
 * histories or the Philox counters, not the presence bitmap (the penalty set stays the FIRST variant plus the generated ids), bias or
 * grammar state.  A finished or parked row never switches.  With key == 1 thresholds are grammar states: under an automaton whose
 * states ascend with musical time (generate_music.grammar.track_grammar: 2 + k ascends with START) the segment follows the START of
 * the row's last note and falls back to segment 0 when a new track opens; key == 0 counts steps. */
#define MGEA_SCHEDULE_MAX_SEGMENTS 8
typedef struct mgea_row_schedule {
    int32_t n_segments;     /* 1 .. 8 prompt variants; 1 = the row never switches */
    int32_t key;            /* 0: the row's step index, 1: its grammar state */
    int32_t threshold[7];   /* ascending (equal values allowed) over [0, n_segments - 1); the rest is not read */
    int32_t reserved;       /* 0 */
} mgea_row_schedule;

/* mgea_decoder_generate_rows_guided with one mgea_row_schedule per row, sched [B] (host memory, read before the call returns), and
 * prompt_ids_dev [n_seg_max][B][Tp].  sched == NULL or n_seg_max == 1 with every n_segments == 1 IS
 * mgea_decoder_generate_rows_guided on variant 0: the same launches and the same ids.  Checked on the host before anything is
 * enqueued: MGEA_EINVAL naming the row for n_segments outside [1, min(8, n_seg_max)], key outside {0, 1}, thresholds that descend or
 * are negative, a non-zero reserved, key == 1 on a row without a start state or with no grammar set, and a guidance shadow row with
 * more than one segment (its prompt has no emotion tokens); MGEA_EINVAL for n_seg_max outside [1, 8] and for a block mode other than
 * the KV-cache one; MGEA_ECAPACITY for Tp > 64.
 * A scheduled call prefills variants n_seg_max - 1 .. 1 and then variant 0 -- each a reset and a prefill of the B prompts, so every
 * variant takes the kernels the generation's own prefill takes --, and copies positions [0, len_b) of every row, layer and head out of
 * the pages into a conditioning store the handle owns after each (n_seg_max * n_layer * B * 2 * d_model * Tp elements; allocated and
 * regrown by scheduled calls only, a regrow synchronises and drops the scheduled graphs).  Every step is then the unscheduled launch
 * sequence of its form behind ONE more launch that applies the rule (after the window's evict launch when windowed); "scheduled" is
 * part of the step-graph key (unscheduled calls capture and replay what they always did), and records, segments and store live in
 * device memory, so other thresholds replay the cached graphs.  It composes with every form, the greedy one included. */
int mgea_decoder_generate_rows_scheduled(mgea_decoder* h, const int32_t* prompt_ids_dev /* [n_seg_max][B][Tp] */, const int32_t* lens_dev,
                                         int32_t B, int32_t Tp, int32_t n_steps, const mgea_row_sampler* rows,
                                         const mgea_row_logits* logits_rows /* NULL ok */,
                                         const int32_t* start_states /* host [B], -1 = none; NULL ok */,
                                         const mgea_row_guidance* guide /* host [B]; NULL ok */,
                                         const mgea_row_schedule* sched /* host [B]; NULL ok */, int32_t n_seg_max,
                                         const int32_t* forced_ids_dev /* NULL ok */, int32_t* ids_out_dev,
                                         float* logprobs_out_dev /* NULL = unscored */, float* choice_logprobs_out_dev /* NULL ok */,
                                         void* stream);
/* out[0] the scheduled decode steps and [1] the switches (rows x times the rule rewrote a row's pages) of the last generation, both
 * 0 if it was not scheduled.  Synchronises `stream`. */
int mgea_decoder_schedule_info(mgea_decoder* h, int64_t* out /* [2] */, void* stream);
/* The rows' current segments cur_seg -> out_dev [B] (device int32).  MGEA_EINVAL if the last generation was not scheduled. */
int mgea_decoder_segments(mgea_decoder* h, int32_t* out_dev, void* stream);

/* Truncation rules beyond top-k and top-p (build-defined in the same sense as top-p: the reference has none; the semantics are
 * HuggingFace's, warper by warper).  At every decode step of a row, steps 1 to 4 of mgea_row_logits run first, then / temperature,
 * top-k and top-p exactly as without a record; the four stages below then apply IN THIS ORDER to the set K kept so far, each seeing
 * p = the softmax over what the stages before it kept:
 *   1. min_p          (MinPLogitsWarper)    remove i where p_i < min_p * max(p);
 *   2. typical_p      (TypicalLogitsWarper) lp = log p, H = -sum_K p_i lp_i, d_i = |-lp_i - H| (p_i = 0 adds nothing to H and has d =
 *                     +inf); d* = the smallest value with mass{i in K : d_i <= d*} >= typical_p, the largest d if even K weighs less;
 *                     keep {i in K : d_i <= d*}.  The row's most likely id is NOT protected (HF's min_tokens_to_keep = 1 protects the
 *                     most typical id there); the id at d* survives, so K never becomes empty;
 *   3. epsilon_cutoff (EpsilonLogitsWarper) remove i where p_i < epsilon; the largest remaining logit always stays (lowest id among
 *                     equals);
 *   4. eta_cutoff     (EtaLogitsWarper)     eta' = min(eta, sqrt(eta) * exp(-H)), H the entropy of the current p; remove i where
 *                     p_i < eta'; the same one-entry protection.
 * The final softmax, the Philox draw, the scored sampler's "choice" log-probability and the tail then run over the final K.  0 switches
 * a stage off, typical_p == 1 too.  A top_k == 1 row stays the exact argmax and ignores the record.  A banned id (-inf) has mass 0 and
 * d = +inf and is never drawn.  H and the normalisers are fixed-order block sums and the typical-p boundary is found over the 2^-40
 * fixed-point masses of top-p, so the same (logits, records, seed, stream, step) give the same id on every run and launch path.
 * Ranges (host check, MGEA_EINVAL naming the row): min_p and typical_p in [0, 1], epsilon_cutoff and eta_cutoff in [0, 1), all finite. */
typedef struct mgea_row_truncation {
    float min_p, typical_p, epsilon_cutoff, eta_cutoff;
} mgea_row_truncation;

/* mgea_decoder_generate_rows_scheduled with one mgea_row_truncation per row, trunc [B] (host memory, read before the call returns).
 * trunc == NULL IS mgea_decoder_generate_rows_scheduled, and a batch in which no non-greedy row has a stage switched on is what it is
 * without the records: the same form, the same graphs, the same ids.  Otherwise the generation is truncated: its steps take the
 * BIASED form at least (GRAMMAR if a row has a start state; presence bitmaps cover every row, a penalty of 1 changes nothing, never
 * the greedy head) with the truncating sampler; "truncated" is part of the step-graph key, and the records live in a device array the
 * handle owns, so a request with other values replays the cached graphs.  A guidance shadow row gets its conditional row's record. */
int mgea_decoder_generate_rows_truncated(mgea_decoder* h, const int32_t* prompt_ids_dev /* [n_seg_max][B][Tp] */, const int32_t* lens_dev,
                                         int32_t B, int32_t Tp, int32_t n_steps, const mgea_row_sampler* rows,
                                         const mgea_row_logits* logits_rows /* NULL ok */,
                                         const int32_t* start_states /* host [B], -1 = none; NULL ok */,
                                         const mgea_row_guidance* guide /* host [B]; NULL ok */,
                                         const mgea_row_schedule* sched /* host [B]; NULL ok */, int32_t n_seg_max,
                                         const int32_t* forced_ids_dev /* NULL ok */, int32_t* ids_out_dev,
                                         float* logprobs_out_dev /* NULL = unscored */, float* choice_logprobs_out_dev /* NULL ok */,
                                         const mgea_row_truncation* trunc /* host [B]; NULL ok */, void* stream);
/* out[0] the truncated decode steps and [1] the rows with a stage switched on of the last generation (both 0 if it was not truncated). */
int mgea_decoder_truncation_info(mgea_decoder* h, int64_t* out /* [2] */);

/* Emotion blends: weighted groups of rows mixed in the sampler (build-defined; the reference returns a distribution over emotions
 * from predict_top_k_labels and has nothing downstream that uses more than its arg-max).  The N-row form of mgea_row_guidance: a
 * GROUP is 2 to MGEA_BLEND_MAX_ROWS rows that name one LEADER -- the same prompt with another emotion's conditioning tokens each --,
 * with member rows m_0 < m_1 < ... < m_{K-1} in ascending row index (the leader wherever it falls) and weights w_k that sum to 1.
 * At every decode step, on the raw head logits of the K rows,
 *   0. (blend) a_k = log_softmax(x_{m_k}), each row's maximum and log-sum-exp reduced exactly as the guidance mix reduces them;
 *      g = w_0 a_0, then g += w_k a_k in ascending k, fp32 (deterministic from run to run); g replaces the logits of ALL K rows;
 *   1.-7. the steps of the guided contract run on g: penalty, bias, grammar, EOS ban, / temperature, top-k, top-p, the truncation
 *      stages, the Philox draw, forced ids and the scored outputs with x := g.
 * One id is drawn per group and fed to all its rows, without a hand-off: before the first step the engine overwrites every
 * non-leader member's sampler record (seed, Philox stream and budget included), truncation record, bias vector, grammar start state,
 * forced ids and -- after the prompts have seeded them -- presence bitmap with its leader's.  A group's repetition-penalty set is
 * therefore the LEADER's prompt plus the generated ids, and what the caller passes in a member's own records is validated and then
 * ignored.  Everything else stays the row's own: its prompt, KV pages, ctx_len and window evictions.  Weights are any finite values
 * (an affine combination: classifier-free guidance is the group (s, 1 - s); a negative weight moves away from a member). */
#define MGEA_BLEND_MAX_ROWS 8
typedef struct mgea_row_blend {
    int32_t leader;   /* the row index of the row's group leader in [0, B); a leader names itself; -1 = the row is in no group */
    float   weight;   /* finite; read only where leader >= 0 */
} mgea_row_blend;

/* mgea_decoder_generate_rows_truncated with one mgea_row_blend per row, blend [B] (host memory, read before the call returns).
 * blend == NULL, or every leader == -1, IS mgea_decoder_generate_rows_truncated: the same launches, the same graphs, the same ids.
 * Checked on the host before anything is enqueued (MGEA_EINVAL naming the row): leader in [-1, B); the named leader names itself; a
 * group has 2 to MGEA_BLEND_MAX_ROWS rows; every weight of a grouped row is finite; a group's weights, summed in double, are within
 * 1e-3 of 1 (a blend is an affine combination, not a hidden temperature); a grouped row is neither the conditional nor the shadow
 * row of a guidance pair and has n_segments == 1.  Pairs and groups on disjoint rows of one batch are allowed: the step then has both
 * launches.  Otherwise the generation is blended: every step is the unblended launch sequence with ONE more launch, the blend mix,
 * between the head GEMM and the sampler; "blended" is part of the step-graph key (unblended calls capture and replay what they always
 * did), and the leaders and weights live in device vectors the handle owns, so a request with other groups or weights replays the
 * cached graphs.  A blended generation never takes the greedy form: all-greedy rows run as top_k == 1 records of the sampled form.
 * ids_out_dev holds every row; a member's line equals its leader's.  Rows outside every group keep the ids they get in an unblended
 * batch of that size and form.  A blended call that would be capped -- Tp + n_steps > max_ctx without a KV window -- is refused with
 * MGEA_ECAPACITY, as a guided one is. */
int mgea_decoder_generate_rows_blended(mgea_decoder* h, const int32_t* prompt_ids_dev /* [n_seg_max][B][Tp] */, const int32_t* lens_dev,
                                       int32_t B, int32_t Tp, int32_t n_steps, const mgea_row_sampler* rows,
                                       const mgea_row_logits* logits_rows /* NULL ok */,
                                       const int32_t* start_states /* host [B], -1 = none; NULL ok */,
                                       const mgea_row_guidance* guide /* host [B]; NULL ok */,
                                       const mgea_row_schedule* sched /* host [B]; NULL ok */, int32_t n_seg_max,
                                       const int32_t* forced_ids_dev /* NULL ok */, int32_t* ids_out_dev,
                                       float* logprobs_out_dev /* NULL = unscored */, float* choice_logprobs_out_dev /* NULL ok */,
                                       const mgea_row_truncation* trunc /* host [B]; NULL ok */,
                                       const mgea_row_blend* blend /* host [B]; NULL ok */, void* stream);
/* out[0] the groups, [1] the grouped rows and [2] the blended decode steps of the last generation (all 0 if it was not blended). */
int mgea_decoder_blend_info(mgea_decoder* h, int64_t* out /* [3] */);

/* Windowed penalties over token CLASSES (build-defined; the reference has only the id-level repetition_penalty).  In this vocabulary
 * an id is a whole note line with its absolute START, so an id recurs only as a literal duplicate: what a listener hears as
 * repetition -- the same pitches, the same rhythm -- lives in attributes of the id.  The engine holds one map class_of [vocab] int32
 * with values in [-1, n_class), 1 <= n_class <= vocab (mgea_decoder_set_penalty_classes); an id of class -1 is in no class: it is
 * never counted and never penalised (instruments, EOS, control tokens).  With the identity map the rule is the frequency_penalty /
 * presence_penalty over ids of other engines.
 * Row b at t = row_step[b], not finished, with a record that is on (frequency != 0 || presence != 0); g_0 .. g_{t-1} the ids the
 * row's steps took (a forced id is a taken id; prompt tokens are conditioning tokens and are NOT counted):
 *   lo  = window > 0 ? max(0, t - window) : 0
 *   n_c = #{ j in [lo, t) : class_of[g_j] == c }, an exact integer (a history entry outside [0, vocab) is skipped)
 *   for every id i with c = class_of[i] >= 0 and n_c > 0, in fp32, three separately rounded operations, never contracted:
 *     m = frequency * (float)n_c;   d = m + presence;   x[i] = x[i] - d
 * and nothing else is written, bit for bit: a finished row, a row whose record is off, t == 0, ids of class -1 and ids of classes
 * with n_c == 0 keep their logits.  This is STEP 0b of the per-step order: behind the guidance and blend mixes of step 0, in front
 * of step 1, the id-level repetition penalty; the result is the row the sampler reads.  In a scored generation logprobs_out is
 * therefore the log-softmax of the class-penalised row, as it is of the mixed row under guidance.  Negative values favour the
 * counted classes.  Under a KV window the counts follow the row's id history, not its cache: tokens whose pages were evicted still
 * count while they are inside `window`.  A guidance shadow row takes its conditional row's record and a blend member its leader's
 * (their histories are the same ids), so the rows of a pair or group keep computing one function. */
#define MGEA_CLASS_PENALTY_MAX_WINDOW 4096
typedef struct mgea_row_class_penalty {
    float   frequency;   /* finite, |.| <= 1e4 */
    float   presence;    /* finite, |.| <= 1e4 */
    int32_t window;      /* the last `window` generated ids are counted; 0 = all of them */
    int32_t reserved;    /* 0 */
} mgea_row_class_penalty;

/* Sets (copies) the class map: class_of_host [vocab] with values in [-1, n_class), 1 <= n_class <= vocab, else MGEA_EINVAL naming
 * the first bad id.  class_of_host == NULL clears it.  The map and the rows' device records are allocated by this call and by nothing
 * else.  Synchronises `stream` and drops the class-penalised step graphs (n_class travels in their kernel arguments). */
int mgea_decoder_set_penalty_classes(mgea_decoder* h, const int32_t* class_of_host, int32_t n_class, void* stream);

/* mgea_decoder_generate_rows_blended with one mgea_row_class_penalty per row, cpen [B] (host memory, read before the call returns).
 * cpen == NULL, or every record off, IS mgea_decoder_generate_rows_blended: the same launches, the same graphs, the same ids.
 * Checked on the host before anything is enqueued (MGEA_EINVAL naming the row): both values finite with |.| <= 1e4; window in
 * [0, MGEA_CLASS_PENALTY_MAX_WINDOW]; reserved == 0; a row that is on with window == 0 needs n_steps <=
 * MGEA_CLASS_PENALTY_MAX_WINDOW; a row that is on needs a class map.  Otherwise every step is the launch sequence it would be
 * with ONE more launch, the class penalty (class_penalty.hip), behind the mixes and in front of the sampler; "class_penalized" is
 * part of the step-graph key, and the records live in a device vector the handle owns, so a request with other values, windows or
 * rows replays the cached graphs.  A class-penalised generation never takes the greedy form: all-greedy rows run as top_k == 1
 * records of the sampled form. */
int mgea_decoder_generate_rows_class_penalized(mgea_decoder* h, const int32_t* prompt_ids_dev /* [n_seg_max][B][Tp] */,
                                               const int32_t* lens_dev, int32_t B, int32_t Tp, int32_t n_steps,
                                               const mgea_row_sampler* rows, const mgea_row_logits* logits_rows /* NULL ok */,
                                               const int32_t* start_states /* host [B], -1 = none; NULL ok */,
                                               const mgea_row_guidance* guide /* host [B]; NULL ok */,
                                               const mgea_row_schedule* sched /* host [B]; NULL ok */, int32_t n_seg_max,
                                               const int32_t* forced_ids_dev /* NULL ok */, int32_t* ids_out_dev,
                                               float* logprobs_out_dev /* NULL = unscored */, float* choice_logprobs_out_dev /* NULL ok */,
                                               const mgea_row_truncation* trunc /* host [B]; NULL ok */,
                                               const mgea_row_blend* blend /* host [B]; NULL ok */,
                                               const mgea_row_class_penalty* cpen /* host [B]; NULL ok */, void* stream);
/* out[0] the n_class of the map that is set (0 = none), [1] the rows that were on and [2] the class-penalised decode steps of the
 * last generation (both 0 if it was not class-penalised). */
int mgea_decoder_class_penalty_info(mgea_decoder* h, int64_t* out /* [3] */);

/* The presence bitmaps of the last penalized generation -> bits_out_dev [B][ceil(vocab / 32)] uint32 (device): bit id & 31 of word
 * id >> 5 of row b is set iff id is in seen_b (including the step at which the row drew eos_id).  MGEA_EINVAL if the last
 * generate applied no penalty (a biased generation keeps the bitmaps too). */
int mgea_decoder_presence(mgea_decoder* h, uint32_t* bits_out_dev, void* stream);

/* The KV window: a generation may run longer than max_ctx (build-defined; the reference's cache simply grows, api_cache.py:159-184).
 * Two of the reference's quirks make it clean: a decode step carries no position information (it adds pos_emb[0]) and no mask, and
 * attention over a set of cached keys does not depend on their order.
 *
 * With a window set, every row of every generation keeps P = sink_pages + ring_pages pages of MGEA_KV_PAGE_TOKENS (64) tokens.  Logical
 * pages 0 .. S-1 are the SINK and are never evicted -- they hold the prompt, the conditioning tokens; pages S .. P-1 are a RING.  A
 * row's ctx_len is then the number of tokens CACHED, no longer the tokens so far; everything else a step records still counts every
 * token: row_step, budgets, min_new_tokens, the Philox counter, the id / log-probability histories and the presence bitmaps (a
 * repetition penalty keeps whole-history semantics).
 *
 * Row b has Lp real prompt tokens; step i (0-based) caches the token it feeds at absolute position Lp + i (step 0 feeds the last
 * prompt token again, as always).
 *   Eviction rule: at the start of a step, a row that is not finished and whose ctx_len == 64 P - 1 evicts its oldest ring page
 *   whole: page_table[b][S .. P-1] rotates left by one (the freed physical page becomes logical page P-1), ctx_len drops by 64 and
 *   the row's eviction counter goes up by one.
 * In closed form, with i0 = 64 P - 1 - Lp: the evictions before step i attends are e(i) = 0 for i < i0 and 1 + (i - i0) div 64
 * otherwise, and step i attends the absolute positions {0 .. 64 S - 1} u {64 (S + e) .. Lp + i}: Lp + i + 1 - 64 e keys, between
 * 64 P - 64 and 64 P - 1 of them once eviction has begun.  Finished rows are left alone: one that finishes at ctx_len = 64 P - 1 reads
 * exactly its P full pages on the later steps of its batch.  (Why 64 P - 1: with the qkv0 table the previous step's tail has already
 * written layer 0's K | V of the fed token at position ctx_len; the rule keeps that write in bounds and alive across the rotation.)
 * The sampled ids of a windowed row depend on (S, R) as well as on what an unwindowed row's depend on.
 *
 * Requirements (MGEA_EINVAL naming the offending value): sink_pages >= 1; ring_pages >= 2 (one ring page would be evicted with the
 * current token's layer-0 K | V in it) and <= 256; sink_pages + ring_pages <= max_ctx / 64; 1 <= max_steps <= MGEA_WINDOW_MAX_STEPS;
 * the KV-cache block mode and MGEA_POS_REFERENCE (an absolute position would be the cached length).  f32 and fp16 engines alike.
 * A windowed generation needs prompt width Tp + 1 <= 64 S (the prompt and its duplicate stay in the sink) and n_steps <= max_steps
 * (MGEA_ECAPACITY otherwise) -- whatever max_ctx is: no budget is clamped and no row is stopped at the end of its pages.  Its
 * histories are a second set with stride max_steps, allocated HERE with the eviction counters (max_batch * max_steps * 16 bytes);
 * mgea_decoder_create allocates nothing for a window.  "Windowed" is part of the step-graph key: every windowed step is the
 * unwindowed launch sequence behind ONE more launch, the eviction, and every page id comes from the page table.  Changing or
 * clearing the window synchronises `stream` and drops the windowed graphs, nothing else.  sink_pages == 0 clears the window: the
 * engine is then exactly the engine without one.
 * After a windowed generation mgea_decoder_step and an extending mgea_decoder_forward are refused (MGEA_EINVAL) until the next
 * mgea_decoder_reset or generate: the host's length tracking no longer holds. */
#define MGEA_WINDOW_MAX_STEPS (1 << 24)
int mgea_decoder_set_window(mgea_decoder* h, int32_t sink_pages, int32_t ring_pages, int32_t max_steps, void* stream);
/* out[0] sink_pages, [1] ring_pages, [2] max_steps of the window set now (all 0: none).  evictions_out (HOST int32 [B], or NULL): the
 * rows' eviction counts of the last generation; synchronises `stream`; MGEA_EINVAL without a window. */
int mgea_decoder_window_info(mgea_decoder* h, int32_t* out /* [3] */, int32_t* evictions_out /* NULL ok */, void* stream);

/* Current cached length of each row -> lens_out_dev [B] (device int32).  Under a KV window (mgea_decoder_set_window) that is the
 * tokens the row's pages hold after its evictions, not the tokens it has seen. */
int mgea_decoder_context_lengths(mgea_decoder* h, int32_t* lens_out_dev, void* stream);
/* Test only: a copy of one layer of the engine's KV pages and of its page table, as the attention reads them (stream-ordered, device to
 * device).  info_out [4] (host): [0] pages per layer, [1] the table's row stride max_pages, [2] bytes per element (4, or 2 on
 * MGEA_DTYPE_F16 engines), [3] bytes of one layer of pages.  pages_out_dev (pages_bytes >= info_out[3]) receives the layer -- page p
 * holds K then V, per head, in the layouts of mgea_op_attention_paged -- and page_table_out_dev [max_batch * max_pages] the table;
 * both NULL: only info_out is filled. */
int mgea_decoder_kv_pages(mgea_decoder* h, int32_t layer, void* pages_out_dev, int64_t pages_bytes, int32_t* page_table_out_dev,
                          int64_t* info_out, void* stream);

/* Per-kernel-class timing for bench.py's roofline leg: with stride n > 0 every n-th decode step of
 * generate() runs eagerly (not from the graph) with a hipEvent pair around each launch, recorded on
 * the launch stream; stride 0 switches it off.  profile_read() synchronises, sums the event pairs
 * into ms_by_class / launches_by_class (classes: 0 gemm, 1 row epilogues, 2 paged attention,
 * 3 dense attention, 4 logits+argmax / sampler; n_classes >= 5) and clears the records. */
int mgea_decoder_profile(mgea_decoder* h, int32_t stride);
int mgea_decoder_profile_read(mgea_decoder* h, double* ms_by_class, int64_t* launches_by_class,
                              int32_t n_classes);

/* out[0] kernels in the step graph last used, [1] graph replays of the last generate(), [2] graph
 * captures + instantiations over the handle's lifetime, [4] graphs cached now, [5] forwards that ran on the f16 matrix-core
 * prefill path (MGEA_DTYPE_F16 engines, empty cache, batch * T big enough: csrc/decoder.hip run_prefill16), [6] decode steps
 * of the last generate() that applied a repetition penalty (0 if it applied none), [7] decode steps of the last generate() that
 * applied a logit bias or min_new_tokens (0 if it applied none), [3] decode steps of the last generate() that wrote log-probabilities
 * (mgea_decoder_generate_rows_scored; 0 otherwise). */
int mgea_decoder_stats(mgea_decoder* h, int64_t* out /* [8] */);
/* Bytes of the engine's layer-0 q | k | v tables (switch decoder_qkv0_table: f32 engines in MGEA_POS_REFERENCE mode, decode steps of at
 * most 64 rows): vocab * 3 * d_model * 4 per decode path that has generated -- one for 3..64 rows, one for 1..2 rows -- and 0 before
 * the first such generation, with the switch off, for every other engine, and for a path whose table found no device memory (that
 * path keeps the layer-0 in-projection launch; nothing fails). */
int mgea_decoder_qkv0_table_bytes(mgea_decoder* h, int64_t* bytes_out);

/* Token ids outside [0, vocab) make nn.Embedding raise IndexError in the reference (api_cache.py:99).
 * Here they are clamped on the device and recorded in a sticky flag word, so that no call has to
 * synchronise to validate its input: this call synchronises `stream`, returns the flags (bit 0 = an id
 * was clamped since the last call; bit 1 = a forced id was banned by the row's grammar state, mgea_decoder_set_grammar) in *flags_out
 * (host) and clears them. */
int mgea_decoder_error_flags(mgea_decoder* h, int32_t* flags_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * DistilBERT(+LoRA) classifier forward: replaces the model call inside
 * emotion_analysis/inference.py:16-20 (transformers DistilBertForSequenceClassification).
 * ------------------------------------------------------------------------------------------ */
typedef struct mgea_bert mgea_bert;

typedef struct mgea_bert_config {
    int32_t vocab, max_pos, dim, n_heads, n_layers, hidden, num_labels;
    int32_t max_tokens; /* B*S capacity of the activation workspace */
    int32_t dtype;      /* MGEA_DTYPE_* */
    float   ln_eps;     /* 1e-12 */
} mgea_bert_config;

/* Arena order (fp32, 256-byte aligned): word_emb[V,D] pos_emb[P,D] emb_ln_w emb_ln_b;
 * per layer (12 tensors): qkv_w[3D,D] (q_lin,k_lin,v_lin rows stacked, LoRA already merged)
 * qkv_b[3D] out_w[D,D] out_b sa_ln_w sa_ln_b lin1_w[Hd,D] lin1_b lin2_w[D,Hd] lin2_b
 * out_ln_w out_ln_b; then pre_w[D,D] pre_b cls_w[labels,D] cls_b. */
int mgea_bert_arena_layout(const mgea_bert_config* cfg, int64_t* offsets_floats, int32_t* n_tensors,
                           int64_t* total_floats);
int mgea_bert_create(const mgea_bert_config* cfg, const float* arena_dev, mgea_bert** out);
int mgea_bert_destroy(mgea_bert* h);
/* ids_dev [B,S] int32, mask_dev [B,S] int32 0/1 or NULL -> logits_out_dev [B,labels] fp32 and/or
 * argmax_out_dev [B] int32 (either may be NULL).  The classifier reads hidden_state[:, 0] of the last layer only: for S >= 4 that layer
 * projects K | V for every position and runs its query, attention, out-projection and FFN for the B [CLS] rows (same logits; switch
 * bert_full_last_layer = 1 computes every position). */
int mgea_bert_forward(mgea_bert* h, const int32_t* ids_dev, const int32_t* mask_dev, int32_t B,
                      int32_t S, float* logits_out_dev, int32_t* argmax_out_dev, void* stream);
/* PACKED forward: the real tokens of the B sequences back to back instead of [B, S] rows padded to the batch's longest
 * prompt (what the tokenizer call of emotion_analysis/inference.py:16 -- padding=True -- hands to the model).  ids_dev / pos_ids_dev
 * [n_tokens] int32 (token id; position of the token inside its sequence), cu_seqlens_dev [B + 1] int32 (sequence b = rows cu[b] ..
 * cu[b + 1] - 1; cu[0] = 0, cu[B] = n_tokens), max_len = the longest sequence.  Every row-wise GEMM, LayerNorm statistic
 * and attention tile then runs on real tokens only; same logits as the padded call with the corresponding prefix mask (a row's results
 * do not depend on the other rows of the batch, and a sequence attends to exactly its own keys in both forms).  Both engine modes take it:
 * F32 engines (and BF16 engines below their 512-token routing threshold) on the exact-fp32 kernels with sequences of any length up to
 * max_pos, BF16 engines from 512 tokens on with sequences of at most 256 tokens.  The caller guarantees a consistent cu_seqlens
 * (non-decreasing, cu[B] = n_tokens, cu[b + 1] - cu[b] in 1..max_len): it is device memory and is not read back. */
int mgea_bert_forward_packed(mgea_bert* h, const int32_t* ids_dev, const int32_t* pos_ids_dev, const int32_t* cu_seqlens_dev, int32_t B,
                             int32_t n_tokens, int32_t max_len, float* logits_out_dev, int32_t* argmax_out_dev, void* stream);
/* Token ids handed over as DEVICE memory are not read back before the forward (that would put a host sync in front of every call):
 * an id outside [0, vocab) -- nn.Embedding raises IndexError in the reference (emotion_analysis/inference.py:16-17) -- is clamped by the
 * embedding kernel and recorded in a sticky device flag.  This call synchronises `stream`, returns the flags (bit 0 = an id was clamped
 * since the last call) in *flags_out (host) and clears them; same contract as mgea_decoder_error_flags. */
int mgea_bert_error_flags(mgea_bert* h, int32_t* flags_out, void* stream);
/* What the handle ran (so that a test can assert WHICH kernels produced the numbers it checks): out[0] forwards so far; of the
 * last forward: [1] 1 = folded-LayerNorm bf16 pipeline, [2] / [3] / [4] bf16 GEMM launches on the persistent 256 x 256 kernel /
 * a ring kernel / the 128 x 128 kernel, [5] persistent launches that cut their left-over tiles into 128-row halves,
 * [6] LayerNorm kernel launches, [7] 1 when the last layer ran for the [CLS] rows only (K | V of every position, the rest on B rows:
 * the classifier reads nothing else; switch bert_full_last_layer = 1 computes every position), [8 + e] bf16 GEMM launches with
 * epilogue e (0..5), [14] rows the GEMMs ran on (padded call: B S; packed call: the real tokens); others 0. */
int mgea_bert_stats(mgea_bert* h, int64_t* out /* [16] */);

/* W[out,in] += scale * B[out,r] @ A[r,in] in place (peft LoRA fold, W' = W + (alpha/r) B A;
 * Scripts/finetuneDistillBert.ipynb:787-795). */
int mgea_lora_merge(float* w_dev, const float* a_dev, const float* b_dev, int32_t out_dim,
                    int32_t in_dim, int32_t r, float scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Op-level entry points (the kernels the engines are built from), exported so the parity
 * tests can check each kernel against the oracle in isolation.  All fp32, row-major.
 * ------------------------------------------------------------------------------------------ */
/* out[M, N] = A[M,K] @ W[N,K]^T, exact-fp32 MFMA, optional split-K (deterministic slab reduce).
 * K % 32 == 0.  workspace_dev: >= mgea_op_gemm_workspace_floats(M,N,split_k) floats. */
int64_t mgea_op_gemm_workspace_floats(int32_t M, int32_t N, int32_t split_k);
int mgea_op_gemm_f32(const float* a_dev, const float* w_dev, const float* bias_dev /* NULL ok */,
                     float* out_dev, int32_t M, int32_t N, int32_t K, int32_t split_k,
                     float* workspace_dev, void* stream);
/* y = LayerNorm(x) over the last dim C (C % 4 == 0, C <= 4096). */
int mgea_op_layernorm(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev,
                      int32_t M, int32_t C, float eps, void* stream);
/* Non-causal attention over a packed qkv buffer [B*T, 3C] (q | k | v, head h at column h*dh);
 * key validity = (t < lens[b] if lens) && (mask[b,t] != 0 if mask).  out [B*T, C]; a row b without a valid key gives zero rows. */
int mgea_op_attention_f32(const float* qkv_dev, const int32_t* lens_dev, const int32_t* mask_dev,
                          float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                          void* stream);
/* The same kernel with every argument its launcher takes (test only).  A query row without a valid key gives a ZERO output row (as
 * mgea_op_attention_cls does), here and above.
 *   cu_seqlens_dev [B + 1] int32 or NULL: packed rows -- qkv / out are [cu[B], 3C / C], sequence b is rows cu[b] .. cu[b + 1] - 1, all
 *               real, T = the longest sequence; refused together with lens_dev, mask_dev or tiled_out.
 *   tiled_out   != 0: out_dev is the k-tiled activation buffer of the fused decode path (mgea_op_tile_rows): whole 64-row groups of
 *               64 * C floats, B * T <= 512 rows; only the floats of rows < B * T are written.
 *   out_dev     caller-provided in both forms; nothing outside the rows above is written (rows t >= lens[b] ARE written). */
int mgea_op_attention_f32_ex(const float* qkv_dev, const int32_t* lens_dev, const int32_t* mask_dev, const int32_t* cu_seqlens_dev,
                             float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim, int32_t tiled_out, void* stream);
/* The causal form of the same kernel (test only; MGEA_POS_CAUSAL engines launch it for a prefill into an empty cache): query i sees the
 * keys t <= i with t < lens_dev[b] (NULL: T).  No mask and no packed rows.  tiled_out and the zero rows of lens_dev[b] == 0 as above.
 * Switch attn_causal_walk: the walk of the grid -- 1 (default) (row, head) pairs fastest and blocks last to first, 2 the non-causal
 * kernel's order, block index fastest. */
int mgea_op_attention_f32_causal(const float* qkv_dev, const int32_t* lens_dev, float* out_dev, int32_t B, int32_t T, int32_t n_head,
                                 int32_t head_dim, int32_t tiled_out, void* stream);
/* out_dev[m] = logits_dev[m * ld + targets_dev[m]] - logsumexp(logits_dev[m * ld .. + V)) for m < M, fp32, the maximum and the sum
 * taken in a fixed order.  targets_dev[m] < 0: out_dev[m] = 0 (row not scored); targets_dev[m] >= V reads entry V - 1.  ld >= V.
 * Stream-ordered, no synchronisation. */
int mgea_op_logprob_gather(const float* logits_dev, int64_t ld, const int32_t* targets_dev, float* out_dev, int32_t M, int32_t V,
                           void* stream);
/* bf16 perf-mode kernels (MGEA_DTYPE_BF16 engines); bf16 buffers are raw 16-bit storage.
 * gemm: out[M,N] = epi(a[M,K] @ w[N,K]^T + bias), fp32 accumulate; epi 0 bias, 1 bias+GELU,
 * 2 bias+residual(res_dev [M,N] bf16).  K % 64 == 0, N % 4 == 0.  attention: head_dim 64 only. */
int mgea_op_f32_to_bf16(const float* src_dev, void* dst_dev, int64_t n, void* stream);
int mgea_op_gemm_bf16(const void* a_dev, const void* w_dev, const float* bias_dev, const void* res_dev,
                      void* out_dev, int32_t M, int32_t N, int32_t K, int32_t epi, void* stream);
/* The same GEMM with the LayerNorm-folding epilogues of the big-batch DistilBERT pipeline (persistent 256 x 256 kernel only:
 * M >= 512, N % 256 == 0; csrc/common.h BfEpiLn), so that the kernel combination the engine picks at B = 256 / S = 128 can be
 * checked in isolation:
 *   epi 3 / 4: out = rstd_row (a w'^T - mean_row c1) + c2 [+ GELU]: a = RAW rows, w' = bf16(W diag(gamma)), bias_dev = c2,
 *              rowstat_dev [M][2] = (mean, rstd) of the a rows (mgea_op_fold_ln_bf16 makes w' / c1 / c2);
 *   epi 5:     out = a w^T + bias + LayerNorm(res row; rowstat_dev, ln_g_dev, ln_b_dev); stats_out_dev [M][N / 256][2] (or NULL)
 *              receives per 256-column tile (sum, M2 about the tile mean) of every output row, which mgea_op_ln_rowstat turns
 *              into the next (mean, rstd);
 *   epi 0..2 as mgea_op_gemm_bf16 (the LayerNorm pointers are ignored).
 * info_out [2] (host, or NULL): [0] the kernel that ran (0 128 x 128 register-staged, 1 ring, 2 persistent), [1] 1 when the
 * persistent kernel cut its left-over tiles into two independent 128-row halves (tiles % CUs <= CUs / 2). */
int mgea_op_gemm_bf16_ln(const void* a_dev, const void* w_dev, const float* bias_dev, const void* res_dev, void* out_dev,
                         int32_t M, int32_t N, int32_t K, int32_t epi, const float* rowstat_dev, const float* c1_dev,
                         const float* ln_g_dev, const float* ln_b_dev, float* stats_out_dev, int32_t* info_out, void* stream);
int mgea_op_ln_rowstat(const float* part_dev, float* rowstat_dev, int32_t M, int32_t n_part, int32_t C, float eps,
                       void* stream);
/* wf_out_dev [N,K] bf16 = bf16(W diag(gamma)); c1[n] = sum_k of the ROUNDED wf[n,k]; c2[n] = bias[n] + sum_k W[n,k] beta[k]. */
int mgea_op_fold_ln_bf16(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, int32_t N,
                         int32_t K, void* wf_out_dev, float* c1_out_dev, float* c2_out_dev, void* stream);
int mgea_op_attention_bf16(const void* qkv_dev, const int32_t* mask_dev, void* out_dev, int32_t B, int32_t T,
                           int32_t n_head, int32_t head_dim, void* stream);
int mgea_op_layernorm_bf16(const void* x_dev, const float* w_dev, const float* b_dev, void* y_dev, int32_t M,
                           int32_t C, float eps, void* stream);
/* The 16-bit kernels of the decoder's fp16 mode (MGEA_DTYPE_F16) and the paged attention, one kernel per call, so that the tests can
 * hold each against exact references instead of the engine's end-to-end tolerances.  `dtype` is MGEA_DTYPE_BF16 or MGEA_DTYPE_F16
 * (16-bit storage) or, for the pages of mgea_op_attention_paged, MGEA_DTYPE_F32.
 * ONE LAYER OF KV PAGES (csrc/common.h KvPool): pages_dev holds n_pages physical pages, page p = [K | V][n_head][64 tokens x head_dim]
 * elements; inside a (p, K|V, head) block K is [head_dim / G][64 tokens][G] and V is [64 tokens][head_dim], G = the elements of a
 * 16-byte group (8 fp16, 4 fp32).  page_table_dev [B][max_pages] int32 names the physical page of logical page j of row b; every entry
 * a call can reach must lie in [0, n_pages) -- checked nowhere, as in the engine, which fills the table itself. */
/* mgea_op_gemm_bf16_ln on fp16 operands: epi 3 / 4 / 5 (fp16 output) and 6 = a w^T + bias as FP32 [M, N] (N % 4 == 0).  Persistent
 * kernel only: M >= 512, N >= 256, at least 8 tiles of 256 x 256; epi 3 / 4 / 5 need N % 256 == 0.  Anything else is MGEA_EINVAL. */
int mgea_op_gemm_f16_ln(const void* a_dev, const void* w_dev, const float* bias_dev, const void* res_dev, void* out_dev,
                        int32_t M, int32_t N, int32_t K, int32_t epi, const float* rowstat_dev, const float* c1_dev,
                        const float* ln_g_dev, const float* ln_b_dev, float* stats_out_dev, int32_t* info_out, void* stream);
/* The two calls above as ONE entry point that can launch what the engines launch: leading dimensions of its own (in elements:
 * a [M, K] with row stride lda, w [N, K] with ldw, out [M, N] with ldc -- fp32 elements for epi 6 -- and res_dev, when given, with
 * the row stride of out), so that a, w and out may be column or row slices of wider buffers (the last DistilBERT layer and the
 * decoder's K | V prefill write N = 2D columns into the middle of a [M, 3D] buffer); f16 != 0: fp16 operands and the rules of
 * mgea_op_gemm_f16_ln, else bf16 and those of mgea_op_gemm_bf16_ln; reverse != 0: ask the persistent kernel to walk every XCD's run
 * of tiles from its end, as the engines' FC2 does (honoured while the switch bf16_gemm_reverse is set; the other kernels ignore it).
 * lda % 8 == 0, ldw % 8 == 0, ldc % 4 == 0 (% 8 for everything but the 128 x 128 kernel), lda >= K, ldw >= K, ldc >= N; the
 * operand pointers 16-byte aligned.  Nothing outside rows [0, M) x columns [0, N) of out is written.
 * info_out [3] (host, or NULL): [0] the kernel family that ran (0 128 x 128 register-staged, 1 ring, 2 persistent, 3 two
 * workgroups per CU), [1] half_tiles as above, [2] the persistent kernel's tail word: bits 0-1 the tail schedule (switch
 * bf16_gemm_tail), bit 2 set when the tiles are walked in reverse (0 for the other families). */
int mgea_op_gemm16(const void* a_dev, int32_t lda, const void* w_dev, int32_t ldw, const float* bias_dev, const void* res_dev, void* out_dev,
                   int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t f16, int32_t reverse, const float* rowstat_dev,
                   const float* c1_dev, const float* ln_g_dev, const float* ln_b_dev, float* stats_out_dev, int32_t* info_out, void* stream);
/* mgea_op_f32_to_bf16 / mgea_op_fold_ln_bf16 with the 16-bit type as an argument (MGEA_DTYPE_BF16: exactly those calls). */
int mgea_op_f32_to_16(const float* src_dev, void* dst_dev, int64_t n, int32_t dtype, void* stream);
int mgea_op_fold_ln_16(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, int32_t N, int32_t K,
                       int32_t dtype, void* wf_out_dev, float* c1_out_dev, float* c2_out_dev, void* stream);
/* The 16-bit flash attention (mgea_op_attention_bf16) in either 16-bit type.  mask_dev [B, T] int32 or NULL.  cu_seqlens_dev [B + 1]
 * int32 or NULL: packed rows (qkv / out [cu[B], 3C / C], T = the longest sequence <= 256, no mask).  pages_dev != NULL (fp16 only,
 * no cu_seqlens): K | V of every key whose mask bit is set (all keys without a mask) are also written to the pages at position t;
 * keys of logical pages >= max_pages are not cached. */
int mgea_op_attention16(const void* qkv_dev, const int32_t* mask_dev, const int32_t* cu_seqlens_dev, void* out_dev, int32_t B, int32_t T,
                        int32_t n_head, int32_t head_dim, int32_t dtype, void* pages_dev, int32_t n_pages,
                        const int32_t* page_table_dev, int32_t max_pages, void* stream);
/* K | V columns of fp16 qkv rows [B * T, 3C] -> fp16 pages: token t < lens[b] (lens_dev NULL: t < T) of row b at position
 * ctx_len_dev[b] + t; positions in logical pages >= max_pages are not cached. */
int mgea_op_kv_scatter_f16(const void* qkv_dev, void* pages_dev, int32_t n_pages, const int32_t* page_table_dev, int32_t max_pages,
                           const int32_t* ctx_len_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                           void* stream);
/* The embedding of the fp16 prefill: x_out_dev [B * T, C] fp16 = f16(tok_emb[id] + pos_emb[pos]), rowstat_out_dev [B * T][2] = (mean,
 * rstd) of the ROUNDED row, mask_out_dev [B * T] int32 (or NULL) = t < lens[b]; rows past lens[b] are zero rows with (0, 1).
 * pos = t (+ ctx_len_dev[b] when absolute_pos and ctx_len_dev), clamped to pos_rows - 1; ids are clamped to the vocabulary and bit 0
 * of *err_flag_dev (or NULL) is set for a clamped REAL token.  C % 4 == 0, C <= 2048. */
int mgea_op_dec_embed_f16(const int32_t* ids_dev, const int32_t* lens_dev, const int32_t* ctx_len_dev, const float* tok_emb_dev,
                          const float* pos_emb_dev, void* x_out_dev, float* rowstat_out_dev, int32_t* mask_out_dev, float eps, int32_t B,
                          int32_t T, int32_t C, int32_t vocab, int32_t pos_rows, int32_t absolute_pos, int32_t* err_flag_dev,
                          void* stream);
/* The decode / extend attention over one layer of pages (dtype MGEA_DTYPE_F32 or MGEA_DTYPE_F16): query (b, t) -- q = columns 0..C-1
 * of row b * T + t of qkv_dev [B * T, 3C] fp32 -- attends to the ctx_len_dev[b] + (lens_dev ? lens_dev[b] : T) cached tokens of row b;
 * out_dev [B * T, C] fp32 row-major, zero rows for t >= lens[b].  arith_batch > 0: the kernel may compute physical page j * arith_batch + b
 * instead of loading the table (which must then say the same); 0: only the table says.  no_split != 0: one workgroup per (row, head,
 * query); otherwise the call brings the split-context scratch (counters zeroed) and the launcher decides as in the engine (switch
 * attn_split).  info_out [1] (host, or NULL): [0] the workgroups per (row, head, query) of the launch, 1 = the unsplit kernel.
 * Synchronises `stream` before it returns. */
int mgea_op_attention_paged(const float* qkv_dev, const void* pages_dev, int32_t n_pages, int32_t dtype, int32_t arith_batch,
                            const int32_t* page_table_dev, int32_t max_pages, const int32_t* ctx_len_dev, const int32_t* lens_dev,
                            float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim, int32_t no_split, int32_t* info_out,
                            void* stream);
/* The same launch with the arguments the engine varies (test only).  pages_dev holds n_layer layers of n_pages pages each, layer l at
 * element l * n_pages * 2 * n_head * 64 * head_dim (the decoder's layer stride); the kernel reads layer `layer`.  tiled_out != 0:
 * out_dev is a k-tiled activation buffer (mgea_op_tile_rows; B * T <= 512 rows), only the floats of rows < B * T are written.
 * split_part_dev / split_count_dev (both or neither; ignored with no_split): the CALLER's split-context scratch, of at least the
 * sizes mgea_op_attn_split_scratch() answers -- part [256 items][16 splits][head_dim + 2] floats (acc[head_dim], max, sum), count
 * [256] int32.  The call neither allocates nor zeroes it: the counters are zeroed once by whoever owns them and every launch leaves
 * them zero; the partials need no initial value.  Without them the call brings its own zeroed scratch, as above.
 * mgea_op_attn_split_count: the launcher's host-side choice of workgroups per (row, head, query) for a launch that has a scratch
 * (switch attn_split; 1 = the unsplit kernel) -- what info_out[0] reports. */
int mgea_op_attn_split_count(int32_t B, int32_t n_head, int32_t T, int32_t max_pages);
int mgea_op_attn_split_scratch(int32_t head_dim, int64_t* part_floats_out, int64_t* count_ints_out);
int mgea_op_attention_paged_ex(const float* qkv_dev, const void* pages_dev, int32_t n_pages, int32_t n_layer, int32_t layer, int32_t dtype,
                               int32_t arith_batch, const int32_t* page_table_dev, int32_t max_pages, const int32_t* ctx_len_dev,
                               const int32_t* lens_dev, float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                               int32_t tiled_out, int32_t no_split, float* split_part_dev, int64_t split_part_floats,
                               int32_t* split_count_dev, int64_t split_count_ints, int32_t* info_out, void* stream);
/* The causal form (test only; MGEA_POS_CAUSAL engines launch it when they extend a cache by T > 1 tokens): query (b, t) attends to the
 * ctx_len_dev[b] + t + 1 tokens up to itself.  T == 1 launches the kernels of mgea_op_attention_paged_ex.  The split-context form is
 * taken for T == 1 only (mgea_op_attn_split_count), so info_out[0] is 1 for every T > 1 and the causal form has no split kernel. */
int mgea_op_attention_paged_causal(const float* qkv_dev, const void* pages_dev, int32_t n_pages, int32_t n_layer, int32_t layer, int32_t dtype,
                                   int32_t arith_batch, const int32_t* page_table_dev, int32_t max_pages, const int32_t* ctx_len_dev,
                                   const int32_t* lens_dev, float* out_dev, int32_t B, int32_t T, int32_t n_head, int32_t head_dim,
                                   int32_t tiled_out, int32_t no_split, float* split_part_dev, int64_t split_part_floats,
                                   int32_t* split_count_dev, int64_t split_count_ints, int32_t* info_out, void* stream);
/* Layouts of the fused decode path.  The skinny GEMM reads both operands in MFMA-fragment order so that
 * every wave load is 1 KB of consecutive bytes (see csrc/common.h):
 *   tile_weights: W [N,K] row-major -> out_dev [mgea_op_tiled_weight_floats(N,K)] (rows padded to 32);
 *   tile_rows:    [M<=512, N] row-major <-> the k-tiled activation buffer (whole 64-row groups of 64 * N floats), to_tiled != 0
 *                 converts row-major -> tiled.  K % 32 == 0, N % 32 == 0. */
int64_t mgea_op_tiled_weight_floats(int32_t N, int32_t K);
int mgea_op_tile_weights(const float* w_dev, int32_t N, int32_t K, float* out_dev, void* stream);
int mgea_op_tile_rows(const float* src_dev, float* dst_dev, int32_t M, int32_t N, int32_t to_tiled, void* stream);
/* LayerNorm folded into the matrix it feeds: wt_out_dev = tiles of gamma[k] * W[n,k], c1[n] = the row sums of those
 * products, c2[n] = sum_k beta[k] * W[n,k] + bias[n], so that LN(x) @ W^T + bias = rstd * (x @ W'^T - mean * c1) + c2. */
int mgea_op_fold_ln(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev,
                    int32_t N, int32_t K, float* wt_out_dev, float* c1_out_dev, float* c2_out_dev, void* stream);
/* Fused skinny GEMM (decode step, M <= 512): out = epilogue(A @ W^T + bias); epi 1 = residual add into out +
 * LayerNorm partial stats, 2 = activation (0 none, 1 GELU, 2 ReLU), 3 = LM head (logits [M,N] row-major in out_dev
 * or NULL, per-tile (max, argmax) partials in stats_out_dev).  a_dev and out_dev are k-tiled activation buffers,
 * w_dev is a tiled weight (above).  Folded LayerNorm of A when ln_c1_dev != NULL: w_dev / ln_c1_dev / bias_dev are
 * mgea_op_fold_ln's wt / c1 / c2 and stats_in_dev [M][n_part][2] holds partial (mean, M2) over part_cnt columns
 * each (n_part even, <= 64).  dbg = 0 (tools/skinny_bench.py, tools/skinny_phases.py). */
int mgea_op_skinny(int32_t epi, const float* a_dev, const float* w_dev, const float* bias_dev,
                   const float* ln_c1_dev, const float* stats_in_dev, int32_t n_part,
                   int32_t part_cnt, float* out_dev, float* stats_out_dev, int32_t M, int32_t N, int32_t K,
                   int32_t act, int32_t dbg, void* stream);
/* Number P of (max, argmax) partials per row that mgea_op_skinny(epi = 3, dbg = 0) of this shape writes, or 0 for a shape it refuses:
 * stats_out_dev receives the maxima as float [row][P] (row stride P) followed, max(64, M) * P floats in, by the int32 argmax indices in
 * the same layout.  (The decode-step head of api_cache.py:105 runs as ONE balanced round of the chip where the shape allows --
 * csrc/head_gemm.hip, P = the CU count -- and on the generic skinny kernel otherwise; switch head_balanced.)  epi = 3 takes no
 * ln_c1_dev. */
int mgea_op_skinny_logits_partials(int32_t M, int32_t N, int32_t K);
/* TEST ONLY: any plan of the decode-step GEMMs (csrc/common.h plan_decode_gemm) on caller buffers, one launch per call, so that the
 * tests can hold each kernel family, instantiation and epilogue against exact references.  The call fills the launcher's argument
 * block from *args, plans, launches exactly that plan and synchronises `stream` before it returns; a shape or combination the plan
 * refuses is MGEA_EINVAL and nothing is launched.  No pointer is range-checked: the caller sizes every buffer as documented here.
 *   family    rowmajor = 1: w_dev is the ROW-MAJOR [N, K] fp32 matrix for the dot-product kernel (csrc/gemv_small.hip: M <= 2,
 *             K % 256 == 0), LayerNorm applied directly from ln_g_dev / ln_b_dev [K] (both or neither; K <= 1024);
 *             rowmajor = 0: w_dev is the tiled copy (mgea_op_tile_weights / mgea_op_fold_ln), LayerNorm folded: ln_c1_dev [N] and
 *             bias_dev = c2, stats_in_dev [M][n_part][2] partial (mean, M2) over part_cnt columns each;
 *   weights   w_f16 = 1 (rowmajor = 0 only): w_dev holds mgea_op_tile_weights_f16's fp16 fragments; with a LayerNorm ln_g_dev [K]
 *             comes next to ln_c1_dev / bias_dev = mgea_op_ln_vectors' c1 / c2 (gamma is applied to the activations);
 *   a_dev     k-tiled activations (mgea_op_tile_rows), whole 64-row groups;
 *   epi       0 QKV:    out_dev [M, N] row-major = q | k | v, N = 3 * n_head * head_dim; K | V of row m = b * T + t (t < lens[b], or
 *                       every t if lens_dev == NULL) are appended at position ctx_len_dev[b] + t of layer `layer` of the page image
 *                       pages_dev: (layer + 1) layers of n_pages pages in the layout above (page_dtype MGEA_DTYPE_F32 / _F16);
 *                       positions in logical pages >= max_pages are not cached; rows past lens[b] are zero rows.  page_table_dev
 *                       [M / T][max_pages].  Needs a LayerNorm;
 *             1 RES:    out_dev = the k-tiled residual stream [M, N], updated in place; stats_out_dev [M][N / 16][2] or NULL (tiled
 *                       family only);
 *             2 ACT:    out_dev k-tiled [M, N] = act(...), act 0 none, 1 GELU, 2 ReLU;
 *             3 LOGITS: out_dev [M, N] row-major or NULL; partials_dev = the (max, argmax) partials in the layout of
 *                       mgea_op_skinny_logits_partials, P = plan_out[10]: the caller brings 2 * max(64, M) * ceil(N / 16) floats, or
 *                       2 * max(64, M) * 512 if that is more (no plan has more partials).
 *   plan_out  [MGEA_DECODE_GEMM_PLAN_INTS] (host) what ran: [0] kind (0 gemm_skinny_kernel, 1 head_balanced_kernel, 2
 *             gemv_rows_kernel), [1] mt, [2] nt, [3] nw, [4] nch, [5] cw, [6] mr, [7] base, [8] grid.x, [9] grid.y, [10] n_partials;
 *             all -1 when the plan was refused. */
#define MGEA_DECODE_GEMM_PLAN_INTS 11
typedef struct mgea_decode_gemm_args {
    int32_t epi, rowmajor, w_f16;
    int32_t M, N, K;
    int32_t act;
    float   eps;
    const float* a_dev;
    const void*  w_dev;
    const float* bias_dev;        /* [N] or NULL */
    const float* ln_c1_dev;
    const float* ln_g_dev;
    const float* ln_b_dev;
    const float* stats_in_dev;
    int32_t n_part, part_cnt;
    float* out_dev;
    float* stats_out_dev;
    /* QKV */
    void*  pages_dev;
    const int32_t* page_table_dev;
    const int32_t* ctx_len_dev;   /* [M / T] */
    const int32_t* lens_dev;      /* [M / T] or NULL */
    int32_t n_pages, page_dtype, n_head, head_dim, layer, max_pages, T;
    int32_t arith_batch;          /* 0: every page id comes from the table; > 0: the pool carries the decoder's allocation rule, logical
                                     page j of row b = physical j * arith_batch + b (the table must agree): >= M / T, max_pages * arith_batch <= n_pages */
    /* LOGITS */
    float* partials_dev;
} mgea_decode_gemm_args;
int mgea_op_decode_gemm(const mgea_decode_gemm_args* args, int32_t* plan_out, void* stream);
/* W [N, K] row-major fp32 -> out_dev: mgea_op_tiled_weight_floats(N, K) fp16 fragments of v_mfma_f32_16x16x32_f16 (rows padded to 32
 * with zeros): per (16-row tile, 32-wide k-chunk) one 1 KB block [lane = 16 g + c][8] holding W[tile * 16 + c][chunk * 32 + 8 g + 0..7],
 * rounded to nearest even. */
int mgea_op_tile_weights_f16(const float* w_dev, int32_t N, int32_t K, void* out_dev, void* stream);
/* The folded-LayerNorm vectors when gamma is applied on the activation side (fp16 tiles): c1[n] = sum_k gamma[k] W[n,k],
 * c2[n] = sum_k beta[k] W[n,k] + bias[n] (bias_dev NULL: + 0), fp64 sums of exact products, rounded once. */
int mgea_op_ln_vectors(const float* w_dev, const float* gamma_dev, const float* beta_dev, const float* bias_dev, int32_t N, int32_t K,
                       float* c1_out_dev, float* c2_out_dev, void* stream);
/* Sampler on a logits matrix [B,V]; step selects the Philox counter: row b draws from counter {b, step, step >> 32, const} under key
 * s->seed (the words, const = 0x6d676561, the key (seed low, seed high) and u = (word 0 >> 8) * 2^-24: mgea_row_sampler; the order of
 * the cumulative sum is unspecified).  probs_out_dev [B,V] or NULL receives the pre-multinomial distribution. */
int mgea_op_sample(const float* logits_dev, int32_t B, int32_t V, const mgea_sampler_config* s,
                   int64_t step, int32_t* ids_out_dev, float* probs_out_dev, void* stream);
/* mgea_op_sample on the repetition-penalized logits (mgea_decoder_generate_penalized): presence_dev [B][ceil(V / 32)] uint32 holds
 * each row's seen ids (bit id & 31 of word id >> 5).  top_k == 1 takes the argmax of the penalized row, ties to the lowest id.
 * repetition_penalty must be finite and > 0; == 1 is mgea_op_sample (presence_dev may then be NULL). */
int mgea_op_sample_penalized(const float* logits_dev, int32_t B, int32_t V, const mgea_sampler_config* s,
                             float repetition_penalty, const uint32_t* presence_dev, int64_t step,
                             int32_t* ids_out_dev, float* probs_out_dev, void* stream);

/* mgea_op_sample with one record per row (rows [B], host): row b reads rows[b] (max_new_tokens and eos_id are ignored) and draws from
 * counter {rows[b].stream, step, step >> 32, const = 0x6d676561} under key rows[b].seed (low half, high half).  presence_dev as in
 * mgea_op_sample_penalized, needed only if some row's repetition_penalty is not 1 (rows with penalty 1 are then unchanged: x * 1 and x / 1 are exact).  top_k == 1 rows take
 * the exact argmax of their (penalized) row, without the temperature division.  Synchronises `stream` before it returns. */
int mgea_op_sample_rows(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                        int64_t step, int32_t* ids_out_dev, float* probs_out_dev, void* stream);
/* mgea_op_sample_rows on the processed logits of mgea_decoder_generate_rows_biased: logits_rows [B] (host) or NULL (then exactly
 * mgea_op_sample_rows).  Row b adds logits_rows[b].bias_dev (V fp32, device) after its penalty and bans rows[b].eos_id (when >= 0)
 * while step < logits_rows[b].min_new_tokens.  The vectors are gathered into a temporary [B][V] buffer; synchronises `stream`. */
int mgea_op_sample_rows_biased(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows,
                               const uint32_t* presence_dev, const mgea_row_logits* logits_rows, int64_t step, int32_t* ids_out_dev,
                               float* probs_out_dev, void* stream);
/* mgea_op_sample_rows_biased as the scored sampler of mgea_decoder_generate_rows_scored runs it (same order of the processing steps,
 * the two values taken at the same places): forced_ids_dev [B] int32 (device) or NULL -- row b takes forced_ids_dev[b] when it is
 * >= 0 (any negative value: the draw decides; >= V: clamped to V - 1 SILENTLY -- this call has no error flags to set, unlike the
 * engine's); logprobs_out_dev [B] = the raw log-probability of ids_out[b], choice_logprobs_out_dev [B] (or NULL)
 * = its log-probability under the distribution in probs_out.  ids_out_dev and logprobs_out_dev are required. */
int mgea_op_sample_rows_scored(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows,
                               const uint32_t* presence_dev, const mgea_row_logits* logits_rows, int64_t step, int32_t* ids_out_dev,
                               float* probs_out_dev, const int32_t* forced_ids_dev, float* logprobs_out_dev,
                               float* choice_logprobs_out_dev, void* stream);
/* mgea_op_sample_rows_biased as the grammar sampler of mgea_decoder_generate_rows_grammar runs it: class_of_dev [V] and next_dev
 * [n_state][n_class] int32 (device, not validated: the caller guarantees mgea_decoder_set_grammar's rules), states_in_dev [B] int32
 * (-1 = the row has no grammar).  Row b with state s >= 0 loses every id whose class s bans before the EOS ban; states_out_dev [B]
 * receives next[s][class_of[id]] for the id it draws (states_in[b] for a row at -1).  Synchronises `stream`. */
int mgea_op_sample_rows_grammar(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                                const mgea_row_logits* logits_rows, const int32_t* class_of_dev, const int32_t* next_dev, int32_t n_state,
                                int32_t n_class, const int32_t* states_in_dev, int64_t step, int32_t* ids_out_dev, float* probs_out_dev,
                                int32_t* states_out_dev, void* stream);
/* One sampler launch as a truncated generation's steps run it (mgea_row_truncation), on caller buffers: trunc [B] (host) or NULL.
 * The other arguments are those of mgea_op_sample_rows_biased, _scored (forced_ids_dev, logprobs_out_dev, choice_logprobs_out_dev; a
 * NULL logprobs_out_dev = unscored, and then the other two must be NULL) and _grammar (class_of_dev NULL = no grammar, and then the
 * other grammar arguments are ignored), in any combination.  trunc == NULL is the op it extends: _grammar, _scored or _biased (the
 * scored grammar launch exists here alone).  With records the launch is the truncating sampler of the form (empty presence bitmaps
 * where presence_dev is NULL and no row is penalized); rows whose stages are all off, and top_k == 1 rows, compute what they compute
 * without it.  Synchronises `stream`. */
int mgea_op_sample_rows_truncated(const float* logits_dev, int32_t B, int32_t V, const mgea_row_sampler* rows, const uint32_t* presence_dev,
                                  const mgea_row_logits* logits_rows /* NULL ok */, const mgea_row_truncation* trunc /* NULL ok */,
                                  int64_t step, int32_t* ids_out_dev, float* probs_out_dev, const int32_t* forced_ids_dev /* NULL ok */,
                                  float* logprobs_out_dev /* NULL = unscored */, float* choice_logprobs_out_dev /* NULL ok */,
                                  const int32_t* class_of_dev /* NULL = no grammar */, const int32_t* next_dev, int32_t n_state,
                                  int32_t n_class, const int32_t* states_in_dev, int32_t* states_out_dev, void* stream);
/* The kernel that opens a windowed decode step (mgea_decoder_set_window, the eviction rule), alone on caller buffers: page_table_dev
 * [B][max_pages], ctx_len_dev / done_dev / evictions_dev [B] int32 (device).  A row with done == 0 and ctx_len == 64 (S + R) - 1
 * rotates its entries [S, S + R) left by one, ctx_len - 64, evictions + 1; every other row is left as it is.  MGEA_EINVAL for
 * sink_pages < 1, ring_pages outside [2, 256] or sink_pages + ring_pages > max_pages. */
int mgea_op_window_evict(int32_t* page_table_dev, int32_t max_pages, int32_t sink_pages, int32_t ring_pages, int32_t* ctx_len_dev,
                         const int32_t* done_dev, int32_t* evictions_dev, int32_t B, void* stream);
/* The guidance mix of a guided decode step (mgea_row_guidance, step 0), alone and IN PLACE on logits_dev [B, V] fp32: for every row c
 * with u = partner_dev[c] in [0, B), g = scale_dev[c] * log_softmax(row c) + (1 - scale_dev[c]) * log_softmax(row u) is written into
 * both rows; every other row is left as it is.  partner_dev int32 [B], scale_dev fp32 [B] (device).  The caller guarantees the pair
 * rules of mgea_decoder_generate_rows_guided and finite logits; V <= 14336, else MGEA_EINVAL. */
int mgea_op_guidance_mix(float* logits_dev, int32_t B, int32_t V, const int32_t* partner_dev, const float* scale_dev, void* stream);
/* The blend mix of a blended decode step (mgea_row_blend, step 0), alone and IN PLACE on logits_dev [B, V] fp32: for every row L with
 * leader_dev[L] == L, the rows with leader_dev[b] == L in ascending order give g = sum_k weight_dev[m_k] * log_softmax(row m_k), added
 * in that order, written into all of them; every other row is left as it is.  leader_dev int32 [B], weight_dev fp32 [B] (device).
 * The caller guarantees the group rules of mgea_decoder_generate_rows_blended and finite logits; V <= 14336, else MGEA_EINVAL. */
int mgea_op_blend_mix(float* logits_dev, int32_t B, int32_t V, const int32_t* leader_dev, const float* weight_dev, void* stream);
/* The class penalty of a class-penalised decode step (mgea_row_class_penalty, step 0b), alone and IN PLACE on logits_dev [B, V] fp32.
 * class_of_dev int32 [V] with values in [-1, n_class); hist_dev int32 [B][stride], row b's taken ids at hist_dev[b * stride + j];
 * row_step_dev / done_dev int32 [B] (device); recs_host [B] (host, checked like a call's records, MGEA_EINVAL naming the row).  The
 * caller guarantees row_step[b] <= stride.  V <= 14336, 1 <= n_class <= V, stride > 0, else MGEA_EINVAL.  Synchronises `stream`. */
int mgea_op_class_penalty(float* logits_dev, int32_t B, int32_t V, const int32_t* class_of_dev, int32_t n_class, const int32_t* hist_dev,
                          int32_t stride, const int32_t* row_step_dev, const int32_t* done_dev, const mgea_row_class_penalty* recs_host,
                          void* stream);
/* The two kernels of a scheduled generation (mgea_row_schedule), alone on caller buffers.  pool_dev: a KV pool
 * [n_layer][n_pages][K | V][H][64 x dh] of fp32 (f16 == 0) or fp16 (f16 == 1) elements in the page layouts of csrc/common.h; row b's
 * logical page 0 is physical page b when arith_batch > 0 and page_table_dev[b * max_pages] otherwise.  store_dev: the conditioning
 * store, n_seg_max * n_layer * B * 2 * H * dh * slot_tokens elements; a row of length len fills the first 2 * H * dh * len elements
 * of its slot (seg, layer, b) in 16-byte groups: first K, group (h * D + dg) * len + t = elements dg * G .. dg * G + G - 1 of token t,
 * head h (G = 4 floats / 8 halves, D = dh / G), then V, group (h * len + t) * D + dg.  meta_dev int32 [4] and len_dev int32 [B] are
 * the layout words {slot_tokens, B, n_seg_max, 0} and the rows' lengths: written by the gather, read by the apply.
 *   gather_seg >= 0: positions [0, lens_dev[b]) (lens_dev NULL: slot_tokens) of every row's page -> the slots of segment gather_seg;
 *   sched_dev != NULL: then the rule of one scheduled step over device vectors: sched_dev [B] records, done_dev, row_step_dev,
 *   gram_state_dev, cur_seg_dev [B] and the counter switches_dev [1].
 * MGEA_EINVAL (nothing launched) for what the launchers refuse: a NULL buffer, head_dim not 32 / 64 / 96, slot_tokens outside
 * [1, 64], n_seg_max outside [1, 8], gather_seg >= n_seg_max, B beyond arith_batch, neither arith_batch nor a table.  The records'
 * values, the page ids and the buffers' sizes are the caller's (the kernels skip a row whose page id or segment is out of range). */
int mgea_op_recondition(void* pool_dev, int32_t n_layer, int32_t n_pages, int32_t H, int32_t dh, int32_t f16, int32_t arith_batch,
                        const int32_t* page_table_dev, int32_t max_pages, void* store_dev, int32_t n_seg_max, int32_t slot_tokens,
                        int32_t* meta_dev, int32_t* len_dev, int32_t B, int32_t gather_seg, const int32_t* lens_dev,
                        const mgea_row_schedule* sched_dev, const int32_t* done_dev, const int32_t* row_step_dev,
                        const int32_t* gram_state_dev, int32_t* cur_seg_dev, int32_t* switches_dev, void* stream);

/* The DistilBERT row, [CLS] and split-K epilogue kernels, one launch per call on caller buffers (tests/test_gpu_bert_kernels.py,
 * tests/test_gpu_attention_exact.py).  No pointer is range-checked: the caller sizes every buffer as documented here. */
/* The [CLS] attention of the last DistilBERT layer (csrc/attn_cls.hip): ONE query per sequence and head against all keys of its
 * sequence.  q_dev [B, D] fp32 (D = n_head * head_dim), qkv_dev [rows, 3 D] (q | k | v; only K | V are read) in kv_dtype MGEA_DTYPE_F32
 * or MGEA_DTYPE_BF16, out_dev [B, D] fp32.  Padded form: sequence b = rows b S .. b S + S - 1, mask_dev [B, S] int32 (0 = key not
 * counted) or NULL.  Packed form: cu_seqlens_dev [B + 1] int32, sequence b = rows cu[b] .. cu[b + 1] - 1, no mask (S is ignored).  A
 * sequence without any valid key gives a zero row.  MGEA_EINVAL: a mask together with cu_seqlens, bf16 with head_dim != 64, head_dim
 * not 32 / 64, any other kv_dtype. */
int mgea_op_attention_cls(const float* q_dev, const void* qkv_dev, int32_t kv_dtype, const int32_t* mask_dev,
                          const int32_t* cu_seqlens_dev, float* out_dev, int32_t B, int32_t S, int32_t n_head, int32_t head_dim,
                          void* stream);
/* out[m] = LayerNorm(word[ids[m]] + pos[t]; ln_w, ln_b, eps) for the B * S rows m, as fp32 or bf16 (out_dtype MGEA_DTYPE_F32 /
 * MGEA_DTYPE_BF16) [B * S, D].  t = m mod S, or pos_ids_dev[m] when pos_ids_dev != NULL (the packed form passes B = rows, S = 1).
 * word_dev [vocab, D], pos_dev [>= every t + 1, D] fp32.  An id outside [0, vocab) is clamped to the nearest row and sets bit 0 of
 * *err_flag_dev (device int32, or NULL: clamped silently).  D % 4 == 0 and D <= 4096 (fp32) / 2048 (bf16), else MGEA_EINVAL. */
int mgea_op_bert_embed(const int32_t* ids_dev, const int32_t* pos_ids_dev, const float* word_dev, const float* pos_dev,
                       const float* ln_w_dev, const float* ln_b_dev, float eps, void* out_dev, int32_t out_dtype, int32_t B, int32_t S,
                       int32_t D, int32_t vocab, int32_t* err_flag_dev, void* stream);
/* The [CLS] rows of h_dev [rows, D] -> out_dev [B, D] fp32: row b S of the padded form, row cu_dev[b] of the packed one (cu_dev
 * [B + 1] int32 or NULL).  dtype MGEA_DTYPE_F32: a copy (D % 4 == 0).  MGEA_DTYPE_BF16 without rowstat_dev: the converted row.
 * MGEA_DTYPE_BF16 with rowstat_dev [rows][2] = (mean, rstd): ((h - mean) rstd) ln_g + ln_b, the folded LayerNorm of the bf16
 * pipeline (ln_g_dev, ln_b_dev [D] required).  rowstat_dev with MGEA_DTYPE_F32 is MGEA_EINVAL. */
int mgea_op_gather_cls(const void* h_dev, int32_t dtype, const float* rowstat_dev, const float* ln_g_dev, const float* ln_b_dev,
                       const int32_t* cu_dev, float* out_dev, int32_t B, int32_t S, int32_t D, void* stream);
/* The fp32 GEMM with the bias / activation epilogue inside the kernel (no split-K, 128 x 128 tiles):
 * out[m, n] = act(sum_k a[m, k] w[n, k] + bias[n]) for n < N, row strides lda / ldw / ldo floats; columns N .. ldo - 1 of out are
 * not written.  act 0 none, 1 GELU, 2 ReLU.  M > 64, N % 4 == 0, K % 32 == 0, lda, ldw >= K, ldo >= N, all three strides multiples
 * of 4, bias_dev required; anything else is MGEA_EINVAL. */
int mgea_op_gemm_f32_direct(const float* a_dev, int32_t lda, const float* w_dev, int32_t ldw, const float* bias_dev, float* out_dev,
                            int32_t ldo, int32_t M, int32_t N, int32_t K, int32_t act, void* stream);
/* The row epilogues of the split-K GEMM on caller-provided slabs: p_dev holds S slabs [M][ldp] fp32, slab s at p_dev + s * ps
 * floats; v[m, n] = sum_s P[s][m][n] (slab order) + bias[n] (bias_dev NULL: + 0).  The kernels load 16 bytes at a time: ldp % 4 == 0,
 * ps % 4 == 0, ldp >= the row length rounded up to 4 (logits_argmax reads scalars: ldp >= V).
 *   bias_act:       out[m, n] = act(v) for n < N, row stride ldo >= N (any value); act 0 none, 1 GELU, 2 ReLU.
 *   bias_res_ln:    post_ln = 0: x[m] += v, and xn[m] = LayerNorm(x[m]) when ln_w_dev != NULL (xn_dev then required);
 *                   post_ln = 1: x[m] = LayerNorm(x[m] + v), ln_w_dev required.  x, xn [M, C]; C % 4 == 0, C <= 4096.
 *   logits_argmax:  logits_dev [M, V] = v (or NULL) and argmax_dev [M] int32 = the LOWEST index of the row maximum (or NULL); a row
 *                   without any value above -inf gives 0.
 *   qkv_scatter:    rows m = b T + t of [B T, 3 C], C = n_head * head_dim (head_dim % 8 == 0).  qkv_out_dev != NULL:
 *                   qkv_out[m] = v for t < lens[b] (lens_dev NULL: every t), zero rows past it, and K | V of those tokens go to
 *                   position ctx_len_dev[b] + t of ONE layer of pages (layout and page table: above; page_dtype MGEA_DTYPE_F32 /
 *                   MGEA_DTYPE_F16).  qkv_out_dev == NULL: scatter only, p_dev is the finished [B T, ldp] buffer (S, ps and bias
 *                   are ignored).  Positions in logical pages >= max_pages are not cached. */
int mgea_op_slab_bias_act(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* out_dev, int32_t ldo,
                          int32_t M, int32_t N, int32_t act, void* stream);
int mgea_op_slab_bias_res_ln(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* x_dev, float* xn_dev,
                             const float* ln_w_dev, const float* ln_b_dev, float eps, int32_t M, int32_t C, int32_t post_ln,
                             void* stream);
int mgea_op_slab_logits_argmax(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* logits_dev,
                               int32_t M, int32_t V, int32_t* argmax_dev, void* stream);
int mgea_op_slab_qkv_scatter(const float* p_dev, int32_t S, int64_t ps, int32_t ldp, const float* bias_dev, float* qkv_out_dev,
                             void* pages_dev, int32_t n_pages, int32_t page_dtype, const int32_t* page_table_dev, int32_t max_pages,
                             const int32_t* ctx_len_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t n_head,
                             int32_t head_dim, void* stream);

/* TEST ONLY: the kernels that END a decode step (csrc/step_tail.hip, the fused tail of csrc/sampler.hip) and the row kernels around the
 * decoder's prefill, one launch per call on caller buffers (tests/test_gpu_step_tail.py; the rule they are held to is written out in
 * tests/step_tail_util.py).  Every call synchronises `stream` before it returns; a shape a launcher refuses is MGEA_EINVAL and nothing is
 * launched.  No pointer is range-checked: the caller sizes every buffer as documented here.
 *
 * mgea_op_step_tail: one end-of-step launch over B rows (1 <= B <= 512), chosen by `kind`:
 *   0  argmax_advance_kernel          (max, argmax) partials -> sampled, the rows' bookkeeping
 *   1  argmax_advance_embed_kernel    the same + the NEXT step's embedding: x (k-tiled) and stats [B][4] = (mean, M2 / 2) x 2, or with
 *                                     qkv0_dev != NULL the table form: x, qkv [B][3 C] = row [fed id] of qkv0 [vocab][3 C], its K | V at
 *                                     position ctx_len (as the next step reads it) of the one-layer page image, no statistics
 *   2  advance_kernel / advance_scored_kernel   sampled_dev is read; presence_dev != NULL: the PENALTY instantiation (bitmaps of
 *                                     ceil(V / 32) words per row); logprob_hist_dev != NULL: the scored kernel files logprob_step_dev /
 *                                     choice_step_dev [B] in logprob_hist_dev / choice_hist_dev [B][hist_stride] (all four required)
 *   3  embed_qkv0_kernel              the table form of kind 1 for ids = cur_ids_dev at ctx_len_dev, no bookkeeping; an id outside
 *                                     [0, vocab) is clamped and sets bit 0 of *err_flag_dev (or NULL)
 *   4  sample_kernel with its fused tail   logits_dev [B][V] (V == vocab), rows required; the instantiation follows the optional parts:
 *                                     presence_dev (PENALTY), logits_rows (BIAS: the rows' vectors are gathered into a temporary [B][V]
 *                                     buffer as in mgea_op_sample_rows_biased), logprob_hist_dev (scored: forced_dev [B] with
 *                                     forced_stride 0 or [B][forced_stride], the histories [B][hist_stride], choice_hist_dev may be
 *                                     NULL, bit 0 of *err_flag_dev for a clamped forced id), class_of_dev (GRAMMAR: next_dev
 *                                     [n_state][n_class], states_dev [B] read and written, done_dev is the rows' finished flags; the
 *                                     allow bitmask is built first by its own kernel, as in mgea_op_sample_rows_grammar; bit 1 of
 *                                     *err_flag_dev for a banned id).  The step index of the draw is row_step_dev[b].
 * The rows' state: cur_ids_dev, ctx_len_dev, done_dev, row_step_dev [B] and n_done_dev [1] int32, ids_out_dev [B][n_steps] or NULL.
 * rows [B] (host) or NULL: with records every row reads its own eos_id and max_new_tokens (0 = no budget; the records are not held to
 * n_steps here) and ctx_cap[b] (host [B] or NULL = no cap) from a temporary device copy of the records the call builds; with NULL the
 * by-value eos_id holds and no row has a budget or a cap.  The embedding (kinds 1, 3, 4): tok_emb_dev [vocab][C], pos_emb_dev
 * [pos_rows][C], x_dev = the k-tiled layout: ceil(B / 64) * 64 * C floats when C % 32 == 0; a width that is no multiple of 32 leaves its
 * last 32-wide k-chunk partly used, so x_dev then needs 64 * round_up(C, 32) floats and holds ONE row group: C % 32 != 0 with B > 64 is
 * MGEA_EINVAL.  C % 4 == 0, C <= 4096, and C <= 1024 with C % head_dim == 0 and
 * fp32 pages (page_dtype MGEA_DTYPE_F32) for the table form, whose page image is ONE layer of n_pages pages with page_table_dev
 * [B][max_pages]; arith_batch > 0 (>= B, max_pages * arith_batch <= n_pages): physical page = j * arith_batch + b, the table is not
 * read.  reserved must be 0. */
typedef struct mgea_step_tail_args {
    int32_t kind, B, n_steps, eos_id;
    int32_t* cur_ids_dev;
    int32_t* ctx_len_dev;
    int32_t* done_dev;
    int32_t* row_step_dev;
    int32_t* n_done_dev;
    int32_t* ids_out_dev;              /* [B][n_steps] or NULL */
    const mgea_row_sampler* rows;      /* host [B] or NULL */
    const int32_t* ctx_cap;            /* host [B] or NULL */
    const mgea_row_logits* logits_rows;/* host [B] or NULL (kind 4) */
    /* partials (kinds 0, 1) */
    const float* pval_dev;             /* [B][n_tiles] */
    const int32_t* pidx_dev;
    int32_t n_tiles;
    int32_t reserved;                  /* 0 */
    int32_t* sampled_dev;              /* [B]: written by kinds 0, 1, 4, read by kind 2 */
    /* the next step's embedding (kinds 1, 3, 4) */
    const float* tok_emb_dev;
    const float* pos_emb_dev;
    float* x_dev;
    float* stats_dev;
    int32_t C, vocab, pos_rows, absolute_pos;
    /* the qkv0 table form */
    const float* qkv0_dev;
    float* qkv_dev;
    void* pages_dev;
    const int32_t* page_table_dev;
    int32_t n_pages, page_dtype, n_head, head_dim, arith_batch, max_pages;
    /* presence and scores (kinds 2, 4) */
    uint32_t* presence_dev;
    int32_t V, hist_stride;
    const float* logprob_step_dev;
    const float* choice_step_dev;
    float* logprob_hist_dev;
    float* choice_hist_dev;
    int32_t* err_flag_dev;
    /* the sampler (kind 4) */
    const float* logits_dev;
    const int32_t* forced_dev;
    int32_t forced_stride, n_state, n_class, reserved2;   /* reserved2: 0 */
    const int32_t* class_of_dev;
    const int32_t* next_dev;
    int32_t* states_dev;
} mgea_step_tail_args;
int mgea_op_step_tail(const mgea_step_tail_args* args, void* stream);
/* The decoder's fp32 prefill embedding of rows m = b T + t: x[m] = tok_emb[ids[m]] + pos_emb[pos], pos = t (+ ctx_len_dev[b] when
 * absolute_pos != 0 and ctx_len_dev != NULL), clamped to pos_rows - 1; rows with t >= lens_dev[b] (NULL: none) are zero rows.  An id
 * outside [0, vocab) is clamped and, for a real row, sets bit 0 of *err_flag_dev (or NULL).  C % 4 == 0, C <= 4096.
 *   form 0 (embed_stats_kernel):  x_out_dev k-tiled, B T <= 512: ceil(B T / 64) * 64 * C floats when C % 32 == 0, else 64 * round_up(C, 32)
 *                                 floats and B T <= 64 (more rows: MGEA_EINVAL, as for mgea_op_step_tail); aux_out_dev = stats [B T][4] = (mean, M2 / 2,
 *                                 mean, M2 / 2) of the row; ln_w_dev / ln_b_dev / eps are ignored;
 *   form 1 (embed_ln_kernel):     x_out_dev [B T][C] row-major, aux_out_dev = xn = LayerNorm(x; ln_w, ln_b, eps) [B T][C]; ln_w_dev ==
 *                                 NULL: x only, aux_out_dev is not touched. */
int mgea_op_dec_embed(int32_t form, const int32_t* ids_dev, const int32_t* lens_dev, const int32_t* ctx_len_dev, const float* tok_emb_dev,
                      const float* pos_emb_dev, float* x_out_dev, float* aux_out_dev, const float* ln_w_dev, const float* ln_b_dev,
                      float eps, int32_t B, int32_t T, int32_t C, int32_t vocab, int32_t pos_rows, int32_t absolute_pos,
                      int32_t* err_flag_dev, void* stream);
/* The bookkeeping launches around a generation, each alone (all arrays int32 / uint32 in device memory):
 *   take_last:      cur_ids[b] = ids[b][n - 1], n = lens[b] (lens_dev NULL: T) clamped to [1, T];
 *   add_lens:       ctx_len[b] += lens[b] (lens_dev NULL: T), unclamped;
 *   presence_seed:  presence[b] (ceil(V / 32) words) = the set of the first n ids of ids[b] (n = lens[b] clamped to [0, T], NULL: T)
 *                   that lie in [0, V); the row is stored whole, so older bits are cleared.  V > 14336 is MGEA_EINVAL;
 *   unpark_rows:    done 2 -> 1 with ctx_len + 1; every other row untouched;
 *   grammar_allow:  allow[s][w] bit k = next[s][32 w + k] >= 0 for 32 w + k < n_class, words = ceil(n_class / 32) per state;
 *                   MGEA_EINVAL unless 1 <= n_state, n_class <= 4096 and n_state * n_class <= 2^20. */
int mgea_op_take_last(const int32_t* ids_dev, const int32_t* lens_dev, int32_t* cur_ids_dev, int32_t B, int32_t T, void* stream);
int mgea_op_add_lens(int32_t* ctx_len_dev, const int32_t* lens_dev, int32_t T, int32_t B, void* stream);
int mgea_op_presence_seed(const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t T, int32_t V, uint32_t* presence_dev,
                          void* stream);
int mgea_op_unpark_rows(int32_t* done_dev, int32_t* ctx_len_dev, int32_t B, void* stream);
int mgea_op_grammar_allow(const int32_t* next_dev, int32_t n_state, int32_t n_class, uint32_t* allow_dev, void* stream);
/* The rows' device records as a generation builds them, read back: rows == NULL: fill_sampler_params_kernel writes B records from *s
 * with stream = b; otherwise the records built from rows [B] (host) are copied.  reserved > 0: clamp_budgets_kernel then sets
 * max_new = min(max_new, reserved - n) with n = lens_dev[b] (NULL: T) clamped to [1, T], and ctx_cap = reserved (T >= reserved is
 * MGEA_EINVAL); reserved == 0: no clamp.  rows_out [B] (host) receives every record in the public form (max_new_tokens = max_new,
 * INT32_MAX = none; repetition_penalty = the record's penalty), ctx_cap_out [B] (host) its ctx_cap (INT32_MAX = none). */
int mgea_op_row_budgets(const mgea_sampler_config* s, const mgea_row_sampler* rows, int32_t B, const int32_t* lens_dev, int32_t T,
                        int32_t reserved, mgea_row_sampler* rows_out, int32_t* ctx_cap_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGEA_H */
