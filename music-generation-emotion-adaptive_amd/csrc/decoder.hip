// Decoder engine behind the C ABI: owns the paged KV pool, activation workspace and the captured
// hipGraph of one decode step.  Replaces GPTWithKV.forward / GPTBlock.forward / sample_kvcache
// (api_cache.py:51-74, 87-106, 159-184); weight names follow remap_state_dict (api_cache.py:118-134).
//
// Reference quirks reproduced on purpose: no attention mask anywhere (prefill is
// bidirectional), every call adds pos_emb[:T] so decode steps always use position row 0, the
// prefill logits are dropped and the first decode step re-feeds the last prompt token (which
// therefore sits in the cache twice).
#include "decoder_handle.h"

using namespace mgea;

namespace {
int arena_layout(const mgea_decoder_config& c, std::vector<int64_t>* offs, int64_t* total) {
    const int64_t V = c.vocab, C = c.d_model, F = c.d_ff, L = c.seq_len;
    std::vector<int64_t> sizes;
    sizes.push_back(V * C);
    sizes.push_back(L * C);
    for (int i = 0; i < c.n_layer; ++i) {
        const int64_t s[L_COUNT] = {C, C, 3 * C * C, 3 * C, C * C, C, C, C, F * C, F, C * F, C};
        for (int j = 0; j < L_COUNT; ++j) sizes.push_back(s[j]);
    }
    sizes.push_back(V * C);
    sizes.push_back(V);
    int64_t o = 0;
    if (offs) offs->clear();
    for (int64_t s : sizes) {
        if (offs) offs->push_back(o);
        o += round_up(s, 64);
    }
    *total = o;
    return (int)sizes.size();
}

int validate(const mgea_decoder_config* c) {
    MGEA_REQUIRE(c, MGEA_EINVAL, "decoder config is NULL");
    MGEA_REQUIRE(c->vocab > 0 && c->seq_len > 0 && c->d_model > 0 && c->n_head > 0 && c->n_layer > 0 && c->d_ff > 0,
                 MGEA_EINVAL, "decoder config: non-positive dimension");
    MGEA_REQUIRE(c->d_model % c->n_head == 0, MGEA_EINVAL, "d_model %d not divisible by n_head %d", c->d_model, c->n_head);
    const int dh = c->d_model / c->n_head;
    // 96 = a 768-wide checkpoint under the reference's hard-coded 8 heads (api_cache.py:112)
    MGEA_REQUIRE(dh == 32 || dh == 64 || dh == 96, MGEA_EINVAL, "head_dim %d not supported (32, 64 or 96)", dh);
    MGEA_REQUIRE(c->d_model % 32 == 0 && c->d_ff % 32 == 0, MGEA_EINVAL, "d_model and d_ff must be multiples of 32");
    MGEA_REQUIRE(c->d_model <= 4096, MGEA_EINVAL, "d_model > 4096 not supported");
    MGEA_REQUIRE(c->max_batch > 0 && c->max_ctx > 0, MGEA_EINVAL, "max_batch / max_ctx must be positive");
    // the sampler keeps a row of logits in registers; refuse at create rather than at the first sampled generate()
    MGEA_REQUIRE(c->vocab <= MGEA_SAMPLER_MAX_VOCAB, MGEA_EINVAL, "vocab %d exceeds the sampler's limit of %d", c->vocab,
                 MGEA_SAMPLER_MAX_VOCAB);
    MGEA_REQUIRE(c->dtype == MGEA_DTYPE_F32 || c->dtype == MGEA_DTYPE_F16, MGEA_EINVAL,
                 "decoder dtype %d not supported (MGEA_DTYPE_F32 or MGEA_DTYPE_F16)", c->dtype);
    MGEA_REQUIRE(c->block_mode == MGEA_BLOCK_PRELN_GELU || c->block_mode == MGEA_BLOCK_POSTLN_RELU, MGEA_EINVAL, "bad block_mode");
    MGEA_REQUIRE(c->pos_mode != MGEA_POS_CAUSAL || c->block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL,
                 "MGEA_POS_CAUSAL needs the KV-cache block mode (the post-LN twin has no cache to extend)");
    if (c->dtype == MGEA_DTYPE_F16) {   // the fp16 mode lives on the fused decode path (tiled fp16 matrices, fp16 KV pages)
        MGEA_REQUIRE(c->block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL, "MGEA_DTYPE_F16 needs the KV-cache block mode");
        MGEA_REQUIRE((c->d_model % 128) == 0 && c->d_model >= 256 && c->d_model <= 1024, MGEA_EINVAL,
                     "MGEA_DTYPE_F16 needs d_model in 256..1024, a multiple of 128 (got %d)", c->d_model);
        MGEA_REQUIRE(dh == 32 || dh == 64, MGEA_EINVAL, "MGEA_DTYPE_F16 needs head_dim 32 or 64 (got %d)", dh);
    }
    return MGEA_OK;
}

int64_t slab_need(const mgea_decoder_config& c, int M) {
    const int C = c.d_model, F = c.d_ff, V = c.vocab;
    const int shapes[5][2] = {{3 * C, C}, {C, C}, {F, C}, {C, F}, {V, C}};
    int64_t need = 0;
    const int Mh = M > 4096 ? 4096 : M;  // the head runs in row chunks of <= 4096
    for (int i = 0; i < 5; ++i) {
        const int m = (i == 4) ? Mh : M;
        const int64_t s = (int64_t)pick_split_k(m, shapes[i][0], shapes[i][1]) * slab_floats(m, shapes[i][0]);
        need = s > need ? s : need;
    }
    return need;
}
}  // namespace

int mgea::ensure_ws(mgea_decoder* h, int64_t M) {
    M = round_up(M, 64);   // the k-tiled buffers of the fused path are whole 64-row groups
    if (M <= h->ws_tokens) return MGEA_OK;
    MGEA_CHECK_HIP(hipDeviceSynchronize());
    DevGroup& g = h->dev_ws;
    g.release();
    h->ws_tokens = h->slab_cap = 0;
    h->graphs.drop_all();  // captured pointers die with the old workspace
    const int C = h->cfg.d_model, F = h->cfg.d_ff;
    int64_t slab = slab_need(h->cfg, (int)M);
    const int64_t s64 = slab_need(h->cfg, 64);
    slab = slab > s64 ? slab : s64;
    auto floats = [&](float** field, int64_t n) {
        if (g.alloc(field, (size_t)n * sizeof(float)) == MGEA_OK) return true;
        set_error("decoder workspace: out of device memory (%lld floats)", (long long)n);
        return false;
    };
    const int64_t fr = M < MGEA_FUSED_MAX_ROWS ? M : MGEA_FUSED_MAX_ROWS;   // rows of the fused path
    const int64_t pcap = fr * ceil_div(h->cfg.vocab, 16);   // every head plan leaves at most one partial per 16 columns (checked in decode_gemm)
    const bool ok = floats(&h->x, M * C) && floats(&h->xn, M * C) && floats(&h->qkv, M * 3 * C) && floats(&h->att, M * C) &&
              floats(&h->hbuf, M * F) && floats(&h->slabs, slab) && floats(&h->logits, (int64_t)h->cfg.max_batch * h->cfg.vocab) &&
              floats(&h->stats, fr * (C / 16 + 1) * 2) && floats(&h->pmax_val, pcap);
    if (!ok || g.alloc(&h->pmax_idx, (size_t)pcap * sizeof(int32_t)) != MGEA_OK) {
        if (ok) set_error("decoder workspace: out of device memory");
        g.release();
        return MGEA_ENOMEM;
    }
    h->slab_cap = slab;
    h->pmax_cap = pcap;
    h->ws_tokens = M;
    return MGEA_OK;
}

namespace {
// gemm + slab bookkeeping
int gemm(mgea_decoder* h, const float* A, int lda, const float* W, int M, int N, int K, int* S, hipStream_t st) {
    const int s = pick_split_k(M, N, K, h->slab_cap);
    MGEA_REQUIRE((int64_t)s * slab_floats(M, N) <= h->slab_cap, MGEA_ECAPACITY, "internal: slab workspace too small");
    ProfScope _ps(h, PC_GEMM, st);
    const int rc = launch_gemm_f32(A, lda, W, K, h->slabs, M, N, K, s, st);
    if (rc < 0) return rc;
    *S = rc;
    return MGEA_OK;
}

// The NL blocks over M = B*T rows.  use_cache_attn: attention over the paged cache (decode /
// extend); otherwise dense attention inside the qkv buffer (prefill with empty cache, twin mode).
// kv_only_last: the caller drops the logits (the prompt prefill of sample_kvcache, api_cache.py:163: `_, past = model(idx)`), so nothing
// reads the last block's output: once its K | V are in the cache the pass is over -- no attention, out-projection or MLP for that block.
int run_blocks(mgea_decoder* h, int B, int T, const int32_t* lens, bool use_cache_attn, bool scatter,
               hipStream_t st, bool kv_only_last = false) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, M = B * T;
    const bool post = c.block_mode == MGEA_BLOCK_POSTLN_RELU;
    for (int l = 0; l < c.n_layer; ++l) {
        int S = 1;
        const float* a_in = post ? h->x : h->xn;
        // big prefill: bias inside the QKV GEMM (qkv written once, no slab) and a scatter that only reads its K | V columns -- 0.5 GB less
        // traffic per block at [64, 1024].  Only where the slab form would not split K either (>= 256 tiles): the same sums.  (Rows past a
        // ragged prompt's length then hold the projection of their padding token instead of zeros; nothing reads them: the attention
        // masks them as keys by `lens` and their own outputs are ignored.)
        if (scatter && M > 64 && (int64_t)ceil_div(M, 128) * ceil_div(3 * C, 128) >= 256) {
            PROF(PC_GEMM, launch_gemm_f32_bias_act(a_in, C, h->lw(l, L_INW), C, h->lw(l, L_INB), h->qkv, 3 * C, M, 3 * C, C, ACT_NONE, st));
            PROF(PC_ROWOP, launch_qkv_scatter(h->qkv, 1, 0, 3 * C, nullptr, nullptr, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
        } else {
        MGEA_TRY(gemm(h, a_in, C, h->lw(l, L_INW), M, 3 * C, C, &S, st));
        if (scatter) {
            PROF(PC_ROWOP, launch_qkv_scatter(h->slabs, S, slab_floats(M, 3 * C), (int)slab_ld(3 * C), h->lw(l, L_INB),
                                        h->qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
        } else {
            PROF(PC_ROWOP, launch_bias_act(h->slabs, S, slab_floats(M, 3 * C), (int)slab_ld(3 * C), h->lw(l, L_INB), h->qkv,
                                     3 * C, M, 3 * C, ACT_NONE, st));
        }
        }
        if (kv_only_last && scatter && l + 1 == c.n_layer) break;
        if (use_cache_attn) {
            PROF(PC_ATTN_PAGED, launch_attn_paged(h->qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, h->att, B, T,
                                       C, 0, st, &h->attn_split, causal(c)));
        } else {
            PROF(PC_ATTN_DENSE, launch_attn_dense(h->qkv, lens, nullptr, h->att, B, T, c.n_head, h->dh, 0, st, nullptr, causal(c)));
        }
        MGEA_TRY(gemm(h, h->att, C, h->lw(l, L_OUTW), M, C, C, &S, st));
        // post-LN: LN1 in place, nothing for a next GEMM to read in xn; pre-LN: x stays raw and xn = LN2(x) feeds fc1
        PROF(PC_ROWOP, launch_bias_res_ln(h->slabs, S, slab_floats(M, C), (int)slab_ld(C), h->lw(l, L_OUTB), h->x, post ? nullptr : h->xn,
                                    h->lw(l, post ? L_LN1W : L_LN2W), h->lw(l, post ? L_LN1B : L_LN2B), c.ln_eps, M, C, post ? 1 : 0, st));
        if (gemm_direct_epilogue_ok((int)M, F)) {   // bias + activation inside the GEMM epilogue (no slab round trip)
            PROF(PC_GEMM, launch_gemm_f32_bias_act(post ? h->x : h->xn, C, h->lw(l, L_FC1W), C, h->lw(l, L_FC1B), h->hbuf, F, M, F,
                                                   C, post ? ACT_RELU : ACT_GELU, st));
        } else {
            MGEA_TRY(gemm(h, post ? h->x : h->xn, C, h->lw(l, L_FC1W), M, F, C, &S, st));
            PROF(PC_ROWOP, launch_bias_act(h->slabs, S, slab_floats(M, F), (int)slab_ld(F), h->lw(l, L_FC1B), h->hbuf, F, M, F,
                                     post ? ACT_RELU : ACT_GELU, st));
        }
        MGEA_TRY(gemm(h, h->hbuf, F, h->lw(l, L_FC2W), M, C, F, &S, st));
        // post-LN: LN2 in place; pre-LN: xn = the next block's LN1(x), none behind the last block
        const bool last = l + 1 == c.n_layer;
        const float* ln_w = post ? h->lw(l, L_LN2W) : last ? nullptr : h->lw(l + 1, L_LN1W);
        const float* ln_b = post ? h->lw(l, L_LN2B) : last ? nullptr : h->lw(l + 1, L_LN1B);
        PROF(PC_ROWOP, launch_bias_res_ln(h->slabs, S, slab_floats(M, C), (int)slab_ld(C), h->lw(l, L_FC2B), h->x, post ? nullptr : h->xn, ln_w,
                                    ln_b, c.ln_eps, M, C, post ? 1 : 0, st));
    }
    return MGEA_OK;
}

// One decode GEMM -- g = 0 in_proj, 1 out_proj, 2 fc1, 3 fc2 of layer l, 4 the head -- on the weights of its family: the arena's
// row-major matrices with LayerNorm applied directly (gv: gemv_rows_kernel) or the tiled copies with LayerNorm folded in.
// `a` brings the activations and the epilogue's buffers; *plan (optional) receives what ran (the head's partial count).
int decode_gemm(mgea_decoder* h, int l, int g, SkinnyArgs a, bool gv, hipStream_t st, DecodeGemmPlan* plan = nullptr) {
    static const int kEpi[5] = {EPI_QKV, EPI_RES, EPI_ACT, EPI_RES, EPI_LOGITS};
    static const int kW[4] = {L_INW, L_OUTW, L_FC1W, L_FC2W}, kB[4] = {L_INB, L_OUTB, L_FC1B, L_FC2B};
    const bool ln = g == 0 || g == 2;
    const int lnw = g == 0 ? L_LN1W : L_LN2W, lnb = g == 0 ? L_LN1B : L_LN2B;
    a.w_f16 = h->f16;
    a.W = g == 4 ? (gv ? h->head_w() : h->head_tw()) : (gv ? h->lw(l, kW[g]) : h->tw(l, g));
    a.bias = g == 4 ? h->head_b() : h->lw(l, kB[g]);
    if (ln && gv) {
        a.ln_g = h->lw(l, lnw); a.ln_b = h->lw(l, lnb);
    } else if (ln) {   // LN(x) @ W^T + b = rstd * (x @ (gamma W)^T - mean * c1) + c2 (launch_ln_fold); fp16 tiles: gamma on A
        a.ln_c1 = g == 0 ? h->qkv_c1(l) : h->fc1_c1(l);
        a.bias = g == 0 ? h->qkv_c2(l) : h->fc1_c2(l);
        if (h->f16) a.ln_g = h->lw(l, lnw);
    }
    DecodeGemmPlan p;
    MGEA_TRY(plan_decode_gemm(kEpi[g], a, gv, &p));
    MGEA_REQUIRE(!a.pmax_val || (int64_t)a.M * p.n_partials <= h->pmax_cap, MGEA_EINVAL,
                 "decoder: %d rows x %d head partials exceed the workspace (%lld)", a.M, p.n_partials, (long long)h->pmax_cap);
    if (plan) *plan = p;
    return launch_decode_gemm(kEpi[g], p, a, st);
}

// qkv0_primed: h->qkv and layer 0's K | V page already hold this step's in-projection of layer 0 (the qkv0 table): that launch is skipped
int run_blocks_fused(mgea_decoder* h, int B, int T, const int32_t* lens, bool use_cache_attn, hipStream_t st,
                     bool kv_only_last = false, bool qkv0_primed = false) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, M = B * T;
    const bool gv = gemv_ok(h, M, T, lens, use_cache_attn);
    int n_part = 2, part_cnt = C / 2;  // the embedding kernel leaves the whole-row statistics as two equal halves
    for (int l = 0; l < c.n_layer; ++l) {
        // ln1 + in_proj + KV append
        SkinnyArgs a{};
        a.M = M; a.eps = c.ln_eps; a.A = h->x; a.lda = C; a.N = 3 * C; a.K = C;
        a.stats_in = h->stats; a.n_part = n_part; a.part_cnt = part_cnt;
        a.out = h->qkv; a.ldo = 3 * C;
        a.pool = kv_view(h); a.layer = l; a.page_table = h->page_table; a.max_pages = h->max_pages; a.ctx_len = h->ctx_len;
        a.lens = lens; a.T = T; a.C = C;
        if (l > 0 || !qkv0_primed) PROF(PC_GEMM, decode_gemm(h, l, 0, a, gv, st));
        if (kv_only_last && l + 1 == c.n_layer) break;       // (run_blocks: the logits are dropped, the last block's K | V are appended)
        if (use_cache_attn) {
            PROF(PC_ATTN_PAGED, launch_attn_paged(h->qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, h->att, B, T, C, 1, st, &h->attn_split, causal(c)));
        } else {
            PROF(PC_ATTN_DENSE, launch_attn_dense(h->qkv, lens, nullptr, h->att, B, T, c.n_head, h->dh, 1, st, nullptr, causal(c)));
        }
        // out_proj + residual (+ stats for ln2)
        SkinnyArgs o{};
        o.M = M; o.eps = c.ln_eps; o.A = h->att; o.lda = C; o.N = C; o.K = C;
        o.out = h->x; o.ldo = C; o.stats_out = h->stats;
        PROF(PC_GEMM, decode_gemm(h, l, 1, o, gv, st));
        n_part = C / 16; part_cnt = 16;
        // ln2 + mlp.0 + GELU
        SkinnyArgs f{};
        f.M = M; f.eps = c.ln_eps; f.A = h->x; f.lda = C; f.N = F; f.K = C;
        f.stats_in = h->stats; f.n_part = n_part; f.part_cnt = part_cnt;
        f.out = h->hbuf; f.ldo = F; f.act = ACT_GELU;
        PROF(PC_GEMM, decode_gemm(h, l, 2, f, gv, st));
        // mlp.2 + residual (+ stats for the next ln1)
        SkinnyArgs r{};
        r.M = M; r.eps = c.ln_eps; r.A = h->hbuf; r.lda = F; r.N = C; r.K = F;
        r.out = h->x; r.ldo = C; r.stats_out = h->stats;
        PROF(PC_GEMM, decode_gemm(h, l, 3, r, gv, st));
    }
    return MGEA_OK;
}

// One decode step (T = 1) of the whole batch.
// kind: the step's launch sequence (StepKind, gen_plan.h); nothing below looks at a sampler setting to choose a kernel.
// pd: the rows' device records (generate()), or NULL and pv by value on every row (mgea_decoder_step).
// primed: x already holds the embedding (+ LN statistics) of cur_ids -- generate() keeps that invariant on the fused path by
// fusing the next step's embedding into this step's tail, so a replayed step is 32 launches.
struct StepCall {
    int B; StepKind kind;
    const SamplerParams* pd; SamplerParams pv;
    float* logits_out;   // optional
    bool primed;
    // primed steps only: the qkv0 table of the step's decode path -- layer 0's q | k | v arrive primed too (no in-projection launch for
    // layer 0) and the tail gathers them for the next step; NULL: the launch
    const float* qkv0 = nullptr;
    // where the head writes the logits row: the caller's buffer, the engine's `own` for the sampler, nowhere for the argmax tails
    float* head_out(float* own) const { return logits_out ? logits_out : (kind.form == StepForm::GREEDY ? nullptr : own); }
};

// What the kernel that embeds the next step's token works on; qkv0: the table of the step's path, or NULL (TailArgs, common.h)
TailArgs tail_args(const mgea_decoder* h, const StepState& s, const float* qkv0) {
    const auto& c = h->cfg;
    TailArgs t{s, h->w(T_TOK), h->w(T_POS), h->x, h->stats, c.d_model, c.vocab, c.seq_len, true_positions(c)};
    if (qkv0) {
        t.qkv0 = qkv0; t.qkv = h->qkv;
        t.pool = kv_view(h); t.page_table = h->page_table; t.max_pages = h->max_pages;
    }
    return t;
}

// The tail of a step over the head's output.  GREEDY: the argmax of the head's n_partials partials per row (0: the ids are already in
// h->sampled), the bookkeeping and, primed, the next step's embedding.  Otherwise the form's sampler over the logits row lg, with the
// bookkeeping and the next embedding as its fused tail when primed, followed by the advance kernel when not.
int enqueue_tail(mgea_decoder* h, const StepCall& k, float* lg, int n_partials, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = k.B, C = c.d_model, V = c.vocab;
    // (with records the EOS id, like the other scalars, is read from them -- the captured graph's form)
    const mgea_decoder::Hist hi = h->hist(k.kind.windowed);
    const StepState s{h->cur_ids, h->ctx_len, h->done, h->row_step, h->n_done, hi.ids, hi.stride, k.pv.eos_id, k.pd};
    const TailArgs t = tail_args(h, s, k.primed ? k.qkv0 : nullptr);
    if (k.kind.form == StepForm::GREEDY) {
        MGEA_REQUIRE(!k.kind.scored && !k.kind.guided && !k.kind.blended && !k.kind.class_penalized, MGEA_EINVAL,
                     "internal: a scored, guided, blended or class-penalised step never takes the greedy form");
        if (k.primed)
            PROF(PC_SAMPLE, launch_argmax_advance_embed(h->pmax_val, h->pmax_idx, n_partials, t, h->sampled, B, st));
        else if (n_partials > 0)
            PROF(PC_SAMPLE, launch_argmax_advance(h->pmax_val, h->pmax_idx, n_partials, s, h->sampled, B, st));
        else
            PROF(PC_ROWOP, launch_advance(h->sampled, s, B, st, nullptr, V));
        return MGEA_OK;
    }
    // guided: every pair's two logits rows become the pair's mixed row, in place, before the sampler reads them
    if (k.kind.guided) PROF(PC_SAMPLE, launch_guidance_mix(lg, B, V, h->guide.partner.d(), h->guide.scale.d(), st));
    // blended: every group's logits rows become the group's mixed row (pairs and groups share no row: either order gives the same rows)
    if (k.kind.blended) PROF(PC_SAMPLE, launch_blend_mix(lg, B, V, h->blend.leader.d(), h->blend.weight.d(), st));
    // class-penalised: behind the mixes (step 0b), every row that is on subtracts its windowed class counts from the row the sampler reads
    if (k.kind.class_penalized)
        PROF(PC_SAMPLE, launch_class_penalty(lg, B, V, h->cpen.class_of, h->cpen.n_class, hi.ids, hi.stride, h->row_step, h->done, h->cpen.rec.d(), st));
    uint32_t* pres = form_has_presence(k.kind.form) ? h->presence : nullptr;
    SampleCall sc{};
    sc.logits = lg; sc.B = B; sc.V = V;
    sc.params_dev = k.pd; sc.params = k.pv; sc.row_step_dev = h->row_step;
    sc.ids_out = h->sampled; sc.tail = k.primed ? &t : nullptr;
    sc.presence = pres; sc.bias = form_has_bias(k.kind.form) ? h->bias : nullptr;
    if (k.kind.form == StepForm::GRAMMAR)
        sc.grammar = GrammarArgs{h->gram.class_of, h->gram.next, h->gram.allow, h->gram.state.d(), h->gram.state.d(), h->done,
                                 h->gram.n_state, h->gram.n_class, grammar_words(h->gram.n_class), h->err_flag};
    if (k.kind.truncated) {
        MGEA_REQUIRE(form_has_bias(k.kind.form), MGEA_EINVAL, "internal: a truncated step takes the biased or the grammar form");
        sc.trunc = TruncArgs{h->trunc.rec.d()};
    }
    const int hs = hi.stride;
    if (k.kind.scored)   // fused tail: the sampler files both values at the row's step; otherwise per-step vectors that advance_kernel files
        sc.score = ScoreArgs{hi.forced, hs, k.primed ? hi.lp : h->lp_step, k.primed ? hi.ch : h->ch_step, hs, h->err_flag};
    PROF(PC_SAMPLE, launch_sample(sc, st));
    const ScoreFile sf{h->lp_step, h->ch_step, hi.lp, hi.ch, hs};
    if (!k.primed) PROF(PC_ROWOP, launch_advance(h->sampled, s, B, st, pres, V, k.kind.scored ? &sf : nullptr));
    return MGEA_OK;
}

// The fused step: [embed,] 6 x (qkv, attention, out-proj, fc1, fc2), head (+ per-tile argmax), tail
int enqueue_step_fused(mgea_decoder* h, const StepCall& k, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = k.B, C = c.d_model, V = c.vocab;
    if (!k.primed)
        PROF(PC_ROWOP, launch_embed_stats(h->cur_ids, nullptr, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->stats, B, 1, C, V,
                                          c.seq_len, true_positions(c), h->err_flag, st));
    MGEA_REQUIRE(!k.qkv0 || k.primed, MGEA_EINVAL, "internal: the qkv0 table serves primed steps only");
    MGEA_TRY(run_blocks_fused(h, B, 1, nullptr, true, st, false, k.qkv0 != nullptr));
    SkinnyArgs a{};
    a.M = B; a.A = h->x; a.lda = C; a.N = V; a.K = C;
    a.out = k.head_out(h->logits);
    a.ldo = V; a.pmax_val = h->pmax_val; a.pmax_idx = h->pmax_idx;
    DecodeGemmPlan head;   // its partial count is what the greedy tail merges
    PROF(PC_GEMM, decode_gemm(h, 0, 4, a, gemv_ok(h, B, 1, nullptr, true) && gemv_shape_ok(B, V, C), st, &head));
    return enqueue_tail(h, k, a.out, head.n_partials, st);
}

// one decode step on cur_ids: the fused path where the geometry has one, else the slab kernels (never primed: they embed cur_ids)
int enqueue_step(mgea_decoder* h, const StepCall& k, hipStream_t st) {
    const auto& c = h->cfg;
    const int B = k.B, C = c.d_model, V = c.vocab;
    const bool post = c.block_mode == MGEA_BLOCK_POSTLN_RELU;
    if (fused_ok(h, B)) return enqueue_step_fused(h, k, st);
    PROF(PC_ROWOP, launch_embed_ln(h->cur_ids, nullptr, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->xn,
                             post ? nullptr : h->lw(0, L_LN1W), post ? nullptr : h->lw(0, L_LN1B), c.ln_eps, B, 1, C,
                             V, c.seq_len, true_positions(c), h->err_flag, st));
    MGEA_TRY(run_blocks(h, B, 1, nullptr, true, true, st));
    int S = 1;
    MGEA_TRY(gemm(h, h->x, C, h->head_w(), B, V, C, &S, st));
    float* lg = k.head_out(h->logits);
    PROF(PC_SAMPLE, launch_logits_argmax(h->slabs, S, slab_floats(B, V), (int)slab_ld(V), h->head_b(), lg, B, V,
                                  k.kind.form == StepForm::GREEDY ? h->sampled : nullptr, st));
    return enqueue_tail(h, k, lg, 0, st);
}
}  // namespace

// Which qkv0 table a primed step of B rows reads: 0 the MFMA kernels', 1 the <= 2-row dot-product kernels', -1 none (the layer-0
// in-projection launch stays).  A constant of the handle and B, so every graph of a batch size has one form.
// The 64-row limit is not technical: tests/test_gpu_decoder.py::test_fused_path_beyond_64_rows pins graph_nodes == 32 for a 100-row f32
// step, and existing tests are this project's yardsticks.  64 rows cover the benchmark and the batched server (RequestBatcher).
int mgea::qkv0_path(const mgea_decoder* h, int B) {
    if (!h->qkv0_on || h->f16 || h->cfg.pos_mode != MGEA_POS_REFERENCE || !fused_ok(h, B) || B > 64) return -1;
    return gemv_ok(h, B, 1, nullptr, true) ? 1 : 0;
}
static const float* qkv0_table(const mgea_decoder* h, int B) {
    const int p = qkv0_path(h, B);
    return p >= 0 && h->qkv0_ready[p] ? h->qkv0_tab[p] : nullptr;
}

// Builds the table of decode path `path` if it is not there: for the ids in chunks of 64 (MFMA) or 2 (GEMV) rows, the embedding at
// position 0 with its statistics, then layer 0's in-projection through decode_gemm -- the step's kernel family and its plan for that
// many rows -- with the chunk's table rows as the output and max_pages = 0, so that the epilogue's page guard keeps it from any KV page.
// The plan of a step is not always the plan of a chunk: pick_mt gives 16-row tiles (MT = 1) to steps of at most 16 rows and to the last,
// short chunk, and 32-row tiles (MT = 2) to the 64-row chunks and to steps of 17..64 rows.  A row's result is the same in both: the
// wave count and the K split do not depend on MT (pick_waves), every 16-row MFMA tile is computed on its own, and the waves' partials are
// added in the same order.  The dot-product kernel likewise computes row 0 of one row and either row of two with the same instruction
// sequence.  tests/test_gpu_qkv0_table.py holds both to the bits (3, 16, 24 and 64 rows; 1 and 2 rows).
// On the call's stream, never inside a capture; x and stats are free between the prefill and the first step.
// Out of device memory: no error, the path keeps its launch (qkv0_no_mem) and mgea_decoder_qkv0_table_bytes says 0.
int mgea::ensure_qkv0(mgea_decoder* h, int path, hipStream_t st) {
    if (h->qkv0_ready[path] || h->qkv0_no_mem[path]) return MGEA_OK;
    const auto& c = h->cfg;
    const int C = c.d_model, V = c.vocab;
    if (!h->qkv0_ids) {
        if (h->dev.alloc(&h->qkv0_ids, ((size_t)V + 64) * sizeof(int32_t))) {
            h->qkv0_no_mem[0] = h->qkv0_no_mem[1] = true;
            return MGEA_OK;
        }
        std::vector<int32_t> iota((size_t)V + 64, 0);
        for (int i = 0; i < V; ++i) iota[(size_t)i] = i;
        MGEA_CHECK_HIP(hipMemcpyAsync(h->qkv0_ids, iota.data(), iota.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        MGEA_CHECK_HIP(hipStreamSynchronize(st));   // iota is a stack-lifetime host buffer (as do_reset's page table)
    }
    if (!h->qkv0_tab[path] && h->dev.alloc(&h->qkv0_tab[path], (size_t)V * 3 * C * sizeof(float))) {
        h->qkv0_no_mem[path] = true;
        return MGEA_OK;
    }
    MGEA_REQUIRE(h->ws_tokens >= 64, MGEA_EINVAL, "internal: qkv0 table build without a 64-row workspace");
    const int rows = path == 1 ? 2 : 64;
    for (int v0 = 0; v0 < V; v0 += rows) {
        const int m = V - v0 < rows ? V - v0 : rows;
        MGEA_TRY(launch_embed_stats(h->qkv0_ids + v0, nullptr, nullptr, h->w(T_TOK), h->w(T_POS), h->x, h->stats, m, 1, C, V, c.seq_len, 0,
                                    nullptr, st));
        SkinnyArgs a{};
        a.M = m; a.eps = c.ln_eps; a.A = h->x; a.lda = C; a.N = 3 * C; a.K = C;
        a.stats_in = h->stats; a.n_part = 2; a.part_cnt = C / 2;
        a.out = h->qkv0_tab[path] + (int64_t)v0 * 3 * C; a.ldo = 3 * C;
        a.pool = h->kv; a.layer = 0; a.page_table = h->page_table; a.max_pages = 0; a.ctx_len = h->qkv0_ids + V;
        a.lens = nullptr; a.T = 1; a.C = C;
        MGEA_TRY(decode_gemm(h, 0, 0, a, path == 1, st));
    }
    h->qkv0_ready[path] = true;
    return MGEA_OK;
}

// The decode step of generate(): the rows' device records; x arrives primed on the fused path.
// windowed: the step opens with the KV window's evict launch, in front of every append of the step (the rule and why it keeps the
// previous tail's layer-0 K | V alive: kv_window.hip); the node does not depend on the step's form.
// guided: the step mixes the pairs' logits rows between the head and the sampler (enqueue_tail); one more node, whatever the pairs are.
// blended: likewise the groups' logits rows, in a launch of its own behind the pairs'; one more node, whatever the groups are.
// class_penalized: the class-penalty launch behind both mixes; one more node, whatever the records are.
// scheduled: behind the evict launch, the launch that applies the rows' prompt schedules (recondition.hip): a row whose segment changes
// gets the new variant's K | V over positions [0, len_b) of its pages before anything of the step reads them; one more node, whatever
// the records say.  (The previous tail's layer-0 K | V of the fed token sits at position ctx_len >= len_b: never in its way.)
int mgea::enqueue_gen_step(mgea_decoder* h, int B, const StepKind& kind, hipStream_t st) {
    if (kind.windowed)
        PROF(PC_ROWOP, launch_window_evict(h->page_table, h->max_pages, h->win.S, h->win.R, h->ctx_len, h->done, h->win.evict, B, st));
    if (kind.scheduled)
        PROF(PC_ROWOP, launch_cond_apply(kv_view(h), h->cfg.n_layer, h->page_table, h->max_pages, h->cond.store, h->cond.meta, h->cond.len,
                                         h->cond.sched.d(), h->done, h->row_step, h->gram.state.d(), h->cond.cur_seg, h->cond.switches, B, st));
    return enqueue_step(h, StepCall{B, kind, h->samp.d(), SamplerParams{}, nullptr, fused_ok(h, B), qkv0_table(h, B)}, st);
}

// embedding (+ LN statistics, or through the qkv0 table) of cur_ids into the buffers the next generate() step will read
int mgea::prime_gen(mgea_decoder* h, int B, hipStream_t st) {
    if (!fused_ok(h, B)) return MGEA_OK;
    const auto& c = h->cfg;
    if (const float* tab = qkv0_table(h, B))
        return launch_embed_qkv0(h->cur_ids, h->ctx_len, tail_args(h, StepState{}, tab), B, h->err_flag, st);
    return launch_embed_stats(h->cur_ids, nullptr, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->stats, B, 1, c.d_model, c.vocab,
                              c.seq_len, true_positions(c), h->err_flag, st);
}

// The captured graph of `steps` decode steps of `kind` over B rows: from the cache, or captured + instantiated now (least recently used
// entry evicted beyond StepGraphs::CAP, hipres.h).
// steps > 1: that many consecutive decode steps in one graph (switch decoder_graph_steps; the per-step state is in device memory, so the
// steps of a graph are as independent of the host as the graphs are of each other)
int mgea::step_graph(mgea_decoder* h, int B, const StepKind& kind, int steps, hipStream_t st, hipGraphExec_t* out) {
    const StepGraphs::Key key{B, steps, kind};
    if (const StepGraphs::Entry* e = h->graphs.find(key)) {
        if (steps == 1) h->n.graph_nodes = e->nodes;
        *out = e->exec;
        return MGEA_OK;
    }
    // the insert below then evicts, and an evicted exec may still be replaying (nothing is launched in between: a capture enqueues no work)
    if (h->graphs.full()) MGEA_CHECK_HIP(hipStreamSynchronize(st));
    MGEA_CHECK_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    int rc = MGEA_OK;
    for (int k = 0; k < steps && rc == MGEA_OK; ++k) rc = enqueue_gen_step(h, B, kind, st);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != MGEA_OK) {
        graph_destroy(g, nullptr);
        return rc;
    }
    MGEA_CHECK_HIP(e);
    hipGraphExec_t ex = nullptr;
    const hipError_t ei = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (ei != hipSuccess) {
        graph_destroy(g, nullptr);
        MGEA_CHECK_HIP(ei);
    }
    size_t nn = 0;
    (void)hipGraphGetNodes(g, nullptr, &nn);
    h->graphs.insert(key, g, ex, (int64_t)nn);
    if (steps == 1) h->n.graph_nodes = (int64_t)nn;
    *out = ex;
    return MGEA_OK;
}

namespace {
// ---- fp16 engines: prefill of a big batch on the f16 matrix cores --------------------------------------------------------------
// The exact-fp32 kernels run a [64, 1024] prefill at 0.67 of THEIR peak, which is 1/16 of the f16 MFMA rate.  When the cache is empty
// and the batch is big enough for the persistent 256 x 256 GEMM (M / 256 * d_model / 256 >= 256 tiles), an fp16 engine runs the GPT
// block (api_cache.py:51-74, 87-106) on the kernels of the bf16 DistilBERT path with _Float16 operands instead:
//   x (fp16) + (mean, rstd) per row  ->  per layer:
//     qkv  = rstd (x W_in'^T - mean c1) + c2            W_in' = f16(W_in diag(ln1 gamma)): LayerNorm folded into the GEMM (epilogue 3)
//     K | V of the real tokens -> fp16 KV pages;  att = flash attention over qkv (non-causal: the reference has no mask), fp16
//     x'   = att W_out^T + b + x, + row statistics      (epilogue 5, identity tables: the residual is the raw x)
//     hid  = gelu(rstd' (x' W_fc1'^T - mean' c1') + c2')  (epilogue 4)
//     x    = hid W_fc2^T + b + x', + row statistics     (epilogue 5)
//   logits = x W_head^T + b as fp32                      (epilogue 6, N = vocab)
// Everything between two GEMM inputs is fp16 (the residual stream too: 11 significant bits, against bf16's 8 in the DistilBERT mode);
// accumulation, LayerNorm statistics and the softmax are fp32.  W_in' / W_fc1' round gamma * f16(W) once more (the decode path applies
// gamma to the activations instead): the two paths serve models that differ by one fp16 rounding of those two matrices -- inside
// the fp16 mode's tolerance (tests/test_gpu_f16.py compares both with the oracle on the rounded matrices).
bool prefill16_ok(const mgea_decoder* h, int64_t M, bool cache_attn, const float* logits_out) {
    const auto& c = h->cfg;
    if (!h->f16 || cache_attn || c.block_mode != MGEA_BLOCK_PRELN_GELU || !tune(TUNE_DECODER_PREFILL16)) return false;
    if (causal(c)) return false;   // attn16.hip has no causal form: a causal engine's prefills stay on the fp32-activation path
    if (h->dh != 64 || c.d_model % 256 != 0 || c.d_ff % 256 != 0 || c.d_model > 2048) return false;
    if (logits_out && c.vocab % 4 != 0) return false;
    // worth it from the size at which the smallest GEMM (N = d_model) fills the chip with 256 x 256 tiles; switch value 2 (tests)
    // takes every size the kernels accept
    const int64_t tiles = (M / 256) * (c.d_model / 256);
    return M >= 512 && M < (1ll << 24) && tiles >= (tune(TUNE_DECODER_PREFILL16) == 2 ? 8 : 256);
}

int ensure_p16(mgea_decoder* h, int64_t M, hipStream_t st) {
    auto& p = h->p16;
    const auto& c = h->cfg;
    const int64_t C = c.d_model, F = c.d_ff, V = c.vocab, NL = c.n_layer;
    if (M > p.rows) {
        MGEA_CHECK_HIP(hipDeviceSynchronize());
        DevGroup& g = h->dev_p16_rows;   // (alloc() answers MGEA_OK = 0: a chain of || stops at the first failure)
        g.release();
        p.rows = 0;
        const int64_t R = round_up(M, 256);
        if (g.alloc(&p.x0, R * C * 2) || g.alloc(&p.x1, R * C * 2) || g.alloc(&p.qkv, R * 3 * C * 2) || g.alloc(&p.att, R * C * 2) ||
            g.alloc(&p.hid, R * F * 2) || g.alloc(&p.rowstat, R * 2 * 4) || g.alloc(&p.stats_part, R * (C / 256) * 2 * 4) ||
            g.alloc(&p.ident, (R * 2 + 2 * C) * 4) || g.alloc(&p.mask, R * 4)) {
            set_error("decoder: out of device memory for the fp16 prefill workspace (%lld tokens)", (long long)M);
            g.release();
            h->dev_p16_mats.release();
            p = mgea_decoder::Prefill16();   // (the matrices too: a prefill that ran out of memory keeps nothing)
            return MGEA_ENOMEM;
        }
        std::vector<float> idv((size_t)(R * 2 + 2 * C), 0.f);       // (0, 1) per row, then C ones (gamma), then C zeros (beta)
        for (int64_t r = 0; r < R; ++r) idv[(size_t)r * 2 + 1] = 1.f;
        for (int64_t d = 0; d < C; ++d) idv[(size_t)(R * 2 + d)] = 1.f;
        struct Guard { DevGroup* g; ~Guard() { if (g) g->release(); } } unless_filled{&g};   // buffers without their table are no workspace: rows stays 0
        MGEA_CHECK_HIP(hipMemcpy(p.ident, idv.data(), idv.size() * 4, hipMemcpyHostToDevice));
        unless_filled.g = nullptr;
        p.rows = R;
    }
    if (!p.weights_ready) {
        if (!p.w || !p.vec) {
            DevGroup& g = h->dev_p16_mats;
            g.release();
            p.w_off.clear();
            int64_t tot = 0;
            for (int l = 0; l < NL; ++l) {
                p.w_off.push_back(tot); tot += 3 * C * C;
                p.w_off.push_back(tot); tot += C * C;
                p.w_off.push_back(tot); tot += F * C;
                p.w_off.push_back(tot); tot += C * F;
            }
            p.w_off.push_back(tot); tot += round_up(V, 256) * C;     // (rows beyond V are never read: the kernel clamps its row index)
            if (g.alloc(&p.w, tot * 2) || g.alloc(&p.vec, NL * (6 * C + 2 * F) * 4)) {
                g.release();   // both or neither: with p.w set and p.vec null the next prefill would skip this block
                p.w_off.clear();
                set_error("decoder: out of device memory for the fp16 prefill matrices");
                return MGEA_ENOMEM;
            }
        }
        for (int l = 0; l < NL; ++l) {
            MGEA_TRY(launch_fold_ln_weights_bf16(h->lw(l, L_INW), h->lw(l, L_LN1W), h->lw(l, L_LN1B), h->lw(l, L_INB), (void*)h->p16_w(4 * l + 0),
                                                 h->p16_vec(l, 0), h->p16_vec(l, 1), (int)(3 * C), (int)C, st, 1));
            MGEA_TRY(launch_f32_to_bf16(h->lw(l, L_OUTW), (void*)h->p16_w(4 * l + 1), C * C, st, 1));
            MGEA_TRY(launch_fold_ln_weights_bf16(h->lw(l, L_FC1W), h->lw(l, L_LN2W), h->lw(l, L_LN2B), h->lw(l, L_FC1B), (void*)h->p16_w(4 * l + 2),
                                                 h->p16_vec(l, 2), h->p16_vec(l, 3), (int)F, (int)C, st, 1));
            MGEA_TRY(launch_f32_to_bf16(h->lw(l, L_FC2W), (void*)h->p16_w(4 * l + 3), C * F, st, 1));
        }
        MGEA_TRY(launch_f32_to_bf16(h->head_w(), (void*)h->p16_w(4 * (int)NL), V * C, st, 1));
        p.weights_ready = true;
    }
    return MGEA_OK;
}

int run_prefill16(mgea_decoder* h, const int32_t* ids, const int32_t* lens, int B, int T, float* logits_out, hipStream_t st, bool kv_only_last) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, V = c.vocab, M = B * T, npart = C / 256;
    MGEA_TRY(ensure_p16(h, M, st));
    auto& p = h->p16;
    void *xc = p.x0, *xo = p.x1;
    const float *id_g = p.ident + p.rows * 2, *id_b = id_g + C;
    PROF(PC_ROWOP, launch_dec_embed_f16(ids, lens, h->ctx_len, h->w(T_TOK), h->w(T_POS), xc, p.rowstat, lens ? p.mask : nullptr, c.ln_eps, B, T,
                                        C, V, c.seq_len, true_positions(c), h->err_flag, st));
    // K | V of the real tokens reach the fp16 KV pages from inside the attention kernel of their layer (attn16.hip: it has those rows in LDS
    // anyway; round 3 ran a scatter kernel per layer that re-read them from the qkv buffer, on a side stream under the attention).  Only a
    // last block that stops at its K | V (kv_only_last: no attention runs) still uses the scatter kernel.
    for (int l = 0; l < c.n_layer; ++l) {
        const bool last = l + 1 == c.n_layer;
        if (last && kv_only_last) {
            // the logits are dropped (run_blocks): of the last block only K | V -- rows C.. of the stacked projection -- then its scatter
            const BfEpiLn qk{p.rowstat, h->p16_vec(l, 0) + C, nullptr, nullptr, nullptr};
            PROF(PC_GEMM, launch_gemm_bf16(xc, C, (const char*)h->p16_w(4 * l + 0) + (int64_t)C * C * 2, C, h->p16_vec(l, 1) + C, nullptr,
                                           (char*)p.qkv + (int64_t)C * 2, 3 * C, M, 2 * C, C, BEPI_LNFOLD, st, nullptr, &qk, 1));
            PROF(PC_ROWOP, launch_kv_scatter_f16(p.qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
            break;
        }
        const BfEpiLn q{p.rowstat, h->p16_vec(l, 0), nullptr, nullptr, nullptr};
        PROF(PC_GEMM, launch_gemm_bf16(xc, C, h->p16_w(4 * l + 0), C, h->p16_vec(l, 1), nullptr, p.qkv, 3 * C, M, 3 * C, C, BEPI_LNFOLD, st, nullptr, &q, 1));
        const KvPages pages{h->kv, l, h->page_table, h->max_pages};
        if (tune(TUNE_DECODER_PREFILL16_PAGES)) {
            PROF(PC_ATTN_DENSE, launch_attn_bf16(p.qkv, lens ? p.mask : nullptr, p.att, B, T, c.n_head, h->dh, st, 1, &pages));
        } else {
            PROF(PC_ROWOP, launch_kv_scatter_f16(p.qkv, h->kv, l, h->page_table, h->max_pages, h->ctx_len, lens, B, T, C, st));
            PROF(PC_ATTN_DENSE, launch_attn_bf16(p.qkv, lens ? p.mask : nullptr, p.att, B, T, c.n_head, h->dh, st, 1));
        }
        const BfEpiLn o{p.ident, nullptr, id_g, id_b, p.stats_part};
        PROF(PC_GEMM, launch_gemm_bf16(p.att, C, h->p16_w(4 * l + 1), C, h->lw(l, L_OUTB), xc, xo, C, M, C, C, BEPI_RES_LN, st, nullptr, &o, 1));
        PROF(PC_ROWOP, launch_ln_rowstat(p.stats_part, p.rowstat, M, npart, C, c.ln_eps, st));
        const BfEpiLn f1{p.rowstat, h->p16_vec(l, 2), nullptr, nullptr, nullptr};
        PROF(PC_GEMM, launch_gemm_bf16(xo, C, h->p16_w(4 * l + 2), C, h->p16_vec(l, 3), nullptr, p.hid, F, M, F, C, BEPI_LNFOLD_GELU, st, nullptr, &f1, 1));
        const BfEpiLn f2{p.ident, nullptr, id_g, id_b, last ? nullptr : p.stats_part};
        // reads FC1's big output: walk the tiles backwards (reverse = 1; gemm16.hip)
        PROF(PC_GEMM, launch_gemm_bf16(p.hid, F, h->p16_w(4 * l + 3), F, h->lw(l, L_FC2B), xo, xc, C, M, C, F, BEPI_RES_LN, st, nullptr, &f2, 1, 1));
        if (!last) PROF(PC_ROWOP, launch_ln_rowstat(p.stats_part, p.rowstat, M, npart, C, c.ln_eps, st));
    }
    if (logits_out)
        PROF(PC_GEMM, launch_gemm_bf16(xc, C, h->p16_w(4 * c.n_layer), C, h->head_b(), nullptr, logits_out, V, M, V, C, BEPI_BIAS_F32, st, nullptr, nullptr, 1));
    h->n.prefill16_forwards += 1;
    return MGEA_OK;
}
}  // namespace

int mgea::do_reset(mgea_decoder* h, int B, int max_len, hipStream_t st) {
    const auto& c = h->cfg;
    MGEA_REQUIRE(B > 0 && B <= c.max_batch, MGEA_ECAPACITY, "batch %d exceeds max_batch %d", B, c.max_batch);
    MGEA_REQUIRE(max_len > 0 && max_len <= c.max_ctx, MGEA_ECAPACITY, "context %d exceeds max_ctx %d", max_len, c.max_ctx);
    const int ppr = ceil_div(max_len, MGEA_KV_PAGE_TOKENS);
    MGEA_REQUIRE((int64_t)B * ppr <= h->kv.n_pages, MGEA_ECAPACITY, "KV pool too small: need %d pages", B * ppr);
    // page allocation: logical page j of row b -> physical j*B + b (the rows' j-th pages are
    // neighbours, so a decode step streams one contiguous region per page index)
    std::vector<int32_t> pt((size_t)c.max_batch * h->max_pages, 0);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < ppr; ++j) pt[(size_t)b * h->max_pages + j] = j * B + b;
    h->kv.arith_batch = B;   // the rule above, for kernels that would rather compute a page id than load it (attn_paged.hip)
    MGEA_CHECK_HIP(hipMemcpyAsync(h->page_table, pt.data(), pt.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));  // pt is a stack-lifetime host buffer
    const size_t nb = (size_t)c.max_batch * sizeof(int32_t);
    for (int32_t* p : {h->ctx_len, h->cur_ids, h->done, h->row_step}) MGEA_CHECK_HIP(hipMemsetAsync(p, 0, nb, st));
    MGEA_CHECK_HIP(hipMemsetAsync(h->n_done, 0, 16, st));
    h->cur_batch = B;
    h->reserved_len = ppr * MGEA_KV_PAGE_TOKENS < c.max_ctx ? ppr * MGEA_KV_PAGE_TOKENS : c.max_ctx;
    h->host_max_len = 0;
    h->host_min_len = 0;
    h->win.dirty = false;
    return MGEA_OK;
}

int mgea::do_forward(mgea_decoder* h, const int32_t* ids, const int32_t* lens, int B, int T, float* logits_out,
               hipStream_t st) {
    const auto& c = h->cfg;
    MGEA_REQUIRE(ids, MGEA_EINVAL, "forward: ids is NULL");
    MGEA_REQUIRE(h->cur_batch > 0, MGEA_EINVAL, "forward: call mgea_decoder_reset first");
    MGEA_REQUIRE(B == h->cur_batch, MGEA_EINVAL, "forward: batch %d differs from the reset batch %d", B, h->cur_batch);
    MGEA_REQUIRE(!h->win.dirty, MGEA_EINVAL, "forward: the cache holds a windowed generation; call mgea_decoder_reset first");
    MGEA_REQUIRE(T > 0, MGEA_EINVAL, "forward: T must be positive");
    // the reference fails with a broadcast RuntimeError when T exceeds the position table (api_cache.py:99)
    MGEA_REQUIRE(T <= c.seq_len, MGEA_EINVAL, "T=%d exceeds the position table (%d rows)", T, c.seq_len);
    const bool post = c.block_mode == MGEA_BLOCK_POSTLN_RELU;
    if (!post)
        MGEA_REQUIRE(h->host_max_len + T <= h->reserved_len, MGEA_ECAPACITY,
                     "context %d + %d new tokens exceeds the reserved %d", h->host_max_len, T, h->reserved_len);
    const int C = c.d_model, V = c.vocab;
    const int64_t M = (int64_t)B * T;
    MGEA_REQUIRE(M < (1ll << 30), MGEA_EINVAL, "forward: too many tokens");
    MGEA_TRY(ensure_ws(h, M));
    const bool cache_attn = (!post) && h->host_max_len > 0;
    const bool p16 = !fused_ok(h, (int)M) && prefill16_ok(h, M, cache_attn, logits_out);
    const bool kv_only_last = !logits_out && !post && !tune(TUNE_DECODER_PREFILL_FULL);   // logits dropped: the last block stops at its K | V
    if (p16) {
        MGEA_TRY(run_prefill16(h, ids, lens, B, T, logits_out, st, kv_only_last));   // computes the logits itself (fp32 output of its head GEMM)
    } else if (fused_ok(h, (int)M)) {
        MGEA_TRY(launch_embed_stats(ids, lens, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->stats, B, T, C, V,
                                    c.seq_len, true_positions(c), h->err_flag, st));
        MGEA_TRY(run_blocks_fused(h, B, T, lens, cache_attn, st, kv_only_last));
    } else {
        MGEA_TRY(launch_embed_ln(ids, lens, h->ctx_len, h->w(T_TOK), h->w(T_POS), h->x, h->xn,
                                 post ? nullptr : h->lw(0, L_LN1W), post ? nullptr : h->lw(0, L_LN1B), c.ln_eps, B, T, C,
                                 V, c.seq_len, (!post) && true_positions(c), h->err_flag, st));
        MGEA_TRY(run_blocks(h, B, T, lens, cache_attn, !post, st, kv_only_last));
    }
    if (p16) {
    } else if (logits_out && fused_ok(h, (int)M)) {
        SkinnyArgs a{};  // x is k-tiled on the fused path: the head is a decode GEMM (LOGITS epilogue) on the tiled weights
        a.M = (int)M; a.A = h->x; a.lda = C; a.N = V; a.K = C;
        a.out = logits_out; a.ldo = V;
        MGEA_TRY(decode_gemm(h, 0, 4, a, false, st));
    } else if (logits_out) {
        for (int64_t r0 = 0; r0 < M; r0 += 4096) {
            const int rows = (int)((M - r0) < 4096 ? (M - r0) : 4096);
            if (V % 4 == 0 && gemm_direct_epilogue_ok(rows, V)) {   // bias inside the GEMM: no slab write + read of rows x V floats.  (Same sums as the slab form wherever that
                                                                    // would not split K: from 256 tiles on.  A remainder chunk of 128..255 tiles used to run with K split; its
                                                                    // logits differ from that form in the last bits of the fp32 sums, within the 5e-6 the long-prompt test observes.)
                PROF(PC_GEMM, launch_gemm_f32_bias_act(h->x + r0 * C, C, h->head_w(), C, h->head_b(), logits_out + r0 * V, V, rows, V, C, ACT_NONE, st));
                continue;
            }
            int S = 1;
            MGEA_TRY(gemm(h, h->x + r0 * C, C, h->head_w(), rows, V, C, &S, st));
            MGEA_TRY(launch_bias_act(h->slabs, S, slab_floats(rows, V), (int)slab_ld(V), h->head_b(),
                                     logits_out + r0 * V, V, rows, V, ACT_NONE, st));
        }
    }
    if (!post) {
        MGEA_TRY(launch_add_lens(h->ctx_len, lens, T, B, st));
        h->host_max_len += T;
    }
    MGEA_TRY(launch_take_last(ids, lens, h->cur_ids, B, T, st));
    return MGEA_OK;
}

extern "C" {

int mgea_decoder_arena_layout(const mgea_decoder_config* cfg, int64_t* offsets_floats, int32_t* n_tensors,
                              int64_t* total_floats) {
    MGEA_TRY(validate(cfg));
    std::vector<int64_t> offs;
    int64_t total = 0;
    const int n = arena_layout(*cfg, &offs, &total);
    if (offsets_floats)
        for (int i = 0; i < n; ++i) offsets_floats[i] = offs[i];
    if (n_tensors) *n_tensors = n;
    if (total_floats) *total_floats = total;
    return MGEA_OK;
}

// (Re)derive the fragment-ordered matrices of the fused decode path from the arena; synchronous.
static int build_tiled_weights(mgea_decoder* h, hipStream_t st) {
    const auto& c = h->cfg;
    const int C = c.d_model, F = c.d_ff, V = c.vocab;
    if (!h->wt) {
        int64_t total = 0;
        h->wt_off.clear();
        for (int l = 0; l < c.n_layer; ++l) {
            h->wt_off.push_back(total); total += wtile_floats(3 * C, C);
            h->wt_off.push_back(total); total += wtile_floats(C, C);
            h->wt_off.push_back(total); total += wtile_floats(F, C);
            h->wt_off.push_back(total); total += wtile_floats(C, F);
        }
        h->wt_off.push_back(total); total += wtile_floats(V, C);
        if (h->dev.alloc(&h->wt, (size_t)total * (h->f16 ? 2 : 4)) || h->dev.alloc(&h->lnv, (size_t)c.n_layer * (6 * C + 2 * F) * sizeof(float))) {
            set_error("decoder_create: allocation of the decode-layout weights (%lld MB) failed", (long long)(total * (h->f16 ? 2 : 4) >> 20));
            return MGEA_ENOMEM;   // (wt may stay without lnv: create destroys the handle, and the check below stops anyone else)
        }
    }
    MGEA_REQUIRE(h->lnv, MGEA_EINVAL, "internal: decode-layout weights half built");
    if (h->f16) {
        // private model copy: the caller's arena with the five matrix kinds rounded to fp16 (fp32 storage) ...
        float* own = h->arena_own;
        MGEA_CHECK_HIP(hipMemcpyAsync(own, h->arena_src, (size_t)h->arena_total * sizeof(float), hipMemcpyDeviceToDevice, st));
        const int mats[4] = {L_INW, L_OUTW, L_FC1W, L_FC2W};
        const int64_t msz[4] = {3ll * C * C, (int64_t)C * C, (int64_t)F * C, (int64_t)C * F};
        for (int l = 0; l < c.n_layer; ++l)
            for (int j = 0; j < 4; ++j) MGEA_TRY(launch_round_f16_inplace(own + h->off[2 + l * L_COUNT + mats[j]], msz[j], st));
        MGEA_TRY(launch_round_f16_inplace(own + h->off[2 + c.n_layer * L_COUNT], (int64_t)V * C, st));
        // ... and its fp16 fragments for the decode path; LayerNorm's gamma is applied on the activation side (gemm_skinny.hip)
        _Float16* wt = static_cast<_Float16*>(h->wt);
        for (int l = 0; l < c.n_layer; ++l) {
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_INW), 3 * C, C, wt + h->wt_off[4 * l + 0], st));
            MGEA_TRY(launch_ln_vectors(h->lw(l, L_INW), h->lw(l, L_LN1W), h->lw(l, L_LN1B), h->lw(l, L_INB), 3 * C, C,
                                       const_cast<float*>(h->qkv_c1(l)), const_cast<float*>(h->qkv_c2(l)), st));
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_OUTW), C, C, wt + h->wt_off[4 * l + 1], st));
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_FC1W), F, C, wt + h->wt_off[4 * l + 2], st));
            MGEA_TRY(launch_ln_vectors(h->lw(l, L_FC1W), h->lw(l, L_LN2W), h->lw(l, L_LN2B), h->lw(l, L_FC1B), F, C,
                                       const_cast<float*>(h->fc1_c1(l)), const_cast<float*>(h->fc1_c2(l)), st));
            MGEA_TRY(launch_tile_weights_f16(h->lw(l, L_FC2W), C, F, wt + h->wt_off[4 * l + 3], st));
        }
        MGEA_TRY(launch_tile_weights_f16(h->head_w(), V, C, wt + h->wt_off[4 * c.n_layer], st));
        MGEA_CHECK_HIP(hipStreamSynchronize(st));
        return MGEA_OK;
    }
    float* wt = static_cast<float*>(h->wt);
    for (int l = 0; l < c.n_layer; ++l) {
        MGEA_TRY(launch_ln_fold(h->lw(l, L_INW), h->lw(l, L_LN1W), h->lw(l, L_LN1B), h->lw(l, L_INB), 3 * C, C,
                                wt + h->wt_off[4 * l + 0], const_cast<float*>(h->qkv_c1(l)), const_cast<float*>(h->qkv_c2(l)), st));
        MGEA_TRY(launch_tile_weights(h->lw(l, L_OUTW), C, C, wt + h->wt_off[4 * l + 1], st));
        MGEA_TRY(launch_ln_fold(h->lw(l, L_FC1W), h->lw(l, L_LN2W), h->lw(l, L_LN2B), h->lw(l, L_FC1B), F, C,
                                wt + h->wt_off[4 * l + 2], const_cast<float*>(h->fc1_c1(l)), const_cast<float*>(h->fc1_c2(l)), st));
        MGEA_TRY(launch_tile_weights(h->lw(l, L_FC2W), C, F, wt + h->wt_off[4 * l + 3], st));
    }
    MGEA_TRY(launch_tile_weights(h->head_w(), V, C, wt + h->wt_off[4 * c.n_layer], st));
    MGEA_CHECK_HIP(hipStreamSynchronize(st));
    return MGEA_OK;
}

int mgea_decoder_create(const mgea_decoder_config* cfg, const float* arena_dev, mgea_decoder** out) {
    MGEA_TRY(validate(cfg));
    MGEA_REQUIRE(arena_dev && out, MGEA_EINVAL, "decoder_create: NULL argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible: the MI355X path has no CPU fallback");
        return MGEA_ENODEVICE;
    }
    { DeviceInfo di; MGEA_TRY(device_info(&di)); }   // cached now: launchers ask for it inside graph capture
    mgea_decoder* h = new mgea_decoder();   // from here on every failure goes through destroy
    h->cfg = *cfg;
    h->arena = h->arena_src = arena_dev;
    h->f16 = cfg->dtype == MGEA_DTYPE_F16;
    int64_t total = 0;
    arena_layout(*cfg, &h->off, &total);
    h->arena_total = total;
    h->dh = cfg->d_model / cfg->n_head;
    h->force_unfused = tune(TUNE_DECODER_UNFUSED) == 1;   // A/B switches (tools/README.md), latched per engine
    h->no_gemv = tune(TUNE_DECODER_NOGEMV) == 1;
    h->no_graph = tune(TUNE_DECODER_NOGRAPH) == 1;
    h->qkv0_on = tune(TUNE_DECODER_QKV0_TABLE) == 1;
    h->pages_per_row_cap = ceil_div(cfg->max_ctx, MGEA_KV_PAGE_TOKENS);
    h->max_pages = h->pages_per_row_cap;
    h->kv.n_pages = cfg->max_batch * h->pages_per_row_cap;
    h->kv.H = cfg->n_head;
    h->kv.dh = h->dh;
    h->kv.f16 = h->f16 ? 1 : 0;
    h->kv.layer_stride = (int64_t)h->kv.n_pages * 2 * cfg->n_head * h->kv.page_elems();
    const size_t pool_bytes = (size_t)h->kv.layer_stride * cfg->n_layer * h->kv.elt_bytes();
    auto fail = [&](int code, const char* what) {
        set_error("decoder_create: %s", what);
        mgea_decoder_destroy(h);
        return code;
    };
    DevGroup& g = h->dev;
    if (h->f16) {
        if (g.alloc(&h->arena_own, (size_t)total * sizeof(float)))
            return fail(MGEA_ENOMEM, "allocation of the fp16-rounded model copy failed");
        h->arena = h->arena_own;   // filled by build_tiled_weights below
    }
    if (cfg->block_mode == MGEA_BLOCK_PRELN_GELU) {
        if (g.alloc(&h->kv.base, pool_bytes)) return fail(MGEA_ENOMEM, "KV pool allocation failed");
        if (hipMemset(h->kv.base, 0, pool_bytes) != hipSuccess) return fail(MGEA_EHIP, "KV pool memset failed");
    }
    const size_t nb = (size_t)cfg->max_batch * sizeof(int32_t), nf = (size_t)cfg->max_batch * sizeof(float);
    h->ids_hist_stride = cfg->max_ctx;
    const size_t nhist = (size_t)cfg->max_batch * h->ids_hist_stride;
    h->attn_split.max_split = MGEA_ATTN_MAX_SPLIT;
    h->attn_split.max_items = MGEA_ATTN_SPLIT_ITEMS;   // attn_split_count(): (row, head) pairs, one query each
    // The state buffers, one list: each at the END of the group, so a feature's buffers come behind those of the features before it and
    // every older buffer keeps the place it had.  fill 0 / 0xff: the bytes the whole buffer starts with; NONE: whatever.
    constexpr int NONE = -1;
    int rc = MGEA_OK;
    auto buf = [&](auto** field, size_t bytes, int fill) {
        if (rc != MGEA_OK) return;
        if (g.alloc(field, bytes)) rc = MGEA_ENOMEM;
        else if (fill != NONE && hipMemset(*field, fill, bytes) != hipSuccess) rc = MGEA_EHIP;
    };
    auto table = [&](auto& t, int fill) {   // a record table: its device array here, its stage in h->pinned
        if (rc != MGEA_OK) return;
        if (t.allocate(g, h->pinned, cfg->max_batch)) rc = MGEA_ENOMEM;
        else if (hipMemset(t.dev, fill, (size_t)cfg->max_batch * t.elt) != hipSuccess) rc = MGEA_EHIP;
    };
    buf(&h->page_table, nb * h->max_pages, 0); buf(&h->ctx_len, nb, 0); buf(&h->cur_ids, nb, 0); buf(&h->done, nb, 0);
    buf(&h->row_step, nb, 0); buf(&h->sampled, nb, NONE); buf(&h->n_done, 16, 0);
    table(h->samp, 0);
    buf(&h->err_flag, 16, 0); buf(&h->presence, (size_t)cfg->max_batch * presence_words(cfg->vocab) * sizeof(uint32_t), NONE);
    buf(&h->ids_hist, nb * h->ids_hist_stride, NONE);
    buf(&h->attn_split.part, (size_t)MGEA_ATTN_SPLIT_ITEMS * MGEA_ATTN_MAX_SPLIT * attn_part_floats(h->dh) * sizeof(float), NONE);
    buf(&h->attn_split.count, MGEA_ATTN_SPLIT_ITEMS * sizeof(int32_t), 0);
    buf(&h->bias, (size_t)cfg->max_batch * cfg->vocab * sizeof(float), NONE); buf(&h->forced, nhist * sizeof(int32_t), 0xff);
    buf(&h->lp_hist, nhist * sizeof(float), NONE); buf(&h->ch_hist, nhist * sizeof(float), NONE); buf(&h->lp_step, nf, NONE); buf(&h->ch_step, nf, NONE);
    table(h->gram.state, 0xff); buf(&h->gram.class_of, (size_t)cfg->vocab * sizeof(int32_t), NONE);
    buf(&h->gram.next, (size_t)MGEA_GRAMMAR_MAX_CELLS * sizeof(int32_t), NONE);
    buf(&h->gram.allow, ((size_t)MGEA_GRAMMAR_MAX_CELLS / 32 + MGEA_GRAMMAR_MAX_STATES) * sizeof(uint32_t), NONE);
    table(h->guide.partner, 0xff); table(h->guide.scale, 0); table(h->trunc.rec, 0); table(h->blend.leader, 0xff); table(h->blend.weight, 0);
    if (rc == MGEA_OK && hipEventCreateWithFlags(&h->stage_free.ev, hipEventDisableTiming) != hipSuccess) rc = MGEA_ENOMEM;
    if (rc != MGEA_OK) return fail(rc, rc == MGEA_ENOMEM ? "state allocation failed" : "state memset failed");
    rc = ensure_ws(h, cfg->max_batch > 64 ? cfg->max_batch : 64);
    if (rc == MGEA_OK && fused_geometry(*cfg)) rc = build_tiled_weights(h, nullptr);
    // (causal engines only, and last in the group: every other engine allocates what it always did, in the same order)
    if (rc == MGEA_OK && causal(*cfg) && g.alloc(&h->lens_m1, nb)) {
        set_error("decoder_create: state allocation failed");
        rc = MGEA_ENOMEM;
    }
    if (rc != MGEA_OK) {
        mgea_decoder_destroy(h);
        return rc;
    }
    *out = h;
    return MGEA_OK;
}

int mgea_decoder_refresh_weights(mgea_decoder* h, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    h->p16.weights_ready = false;   // rebuilt from the refreshed model copy at the next big-batch prefill
    h->qkv0_ready[0] = h->qkv0_ready[1] = false;   // and the qkv0 tables at the next generation, in place (the graphs keep their pointers)
    if (!fused_geometry(h->cfg)) return MGEA_OK;
    return build_tiled_weights(h, (hipStream_t)stream);
}

int mgea_decoder_destroy(mgea_decoder* h) {
    if (!h) return MGEA_OK;
    (void)hipDeviceSynchronize();
    delete h;   // every resource goes with its owner (devmem.h, hipres.h)
    return MGEA_OK;
}

int mgea_decoder_reset(mgea_decoder* h, int32_t batch, int32_t max_len, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    return do_reset(h, batch, max_len, (hipStream_t)stream);
}

int mgea_decoder_forward(mgea_decoder* h, const int32_t* ids_dev, const int32_t* lens_dev, int32_t B, int32_t T,
                         float* logits_out_dev, void* stream) {
    MGEA_REQUIRE(h, MGEA_EINVAL, "decoder handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    return do_forward(h, ids_dev, lens_dev, B, T, logits_out_dev, (hipStream_t)stream);
}

int mgea_decoder_step(mgea_decoder* h, const int32_t* ids_in_dev, const mgea_sampler_config* s, int32_t* ids_out_dev,
                      float* logits_out_dev, void* stream) {
    MGEA_REQUIRE(h && s, MGEA_EINVAL, "decoder_step: NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    hipStream_t st = (hipStream_t)stream;
    MGEA_REQUIRE(h->cfg.block_mode == MGEA_BLOCK_PRELN_GELU, MGEA_EINVAL, "decoder_step needs the KV-cache block mode");
    MGEA_REQUIRE(h->cur_batch > 0, MGEA_EINVAL, "decoder_step: call reset/forward first");
    MGEA_REQUIRE(!h->win.dirty, MGEA_EINVAL, "decoder_step: the cache holds a windowed generation; call mgea_decoder_reset first");
    MGEA_REQUIRE(h->host_max_len + 1 <= h->reserved_len, MGEA_ECAPACITY, "context %d + 1 exceeds the reserved %d",
                 h->host_max_len, h->reserved_len);
    const int B = h->cur_batch;
    if (ids_in_dev)
        MGEA_CHECK_HIP(hipMemcpyAsync(h->cur_ids, ids_in_dev, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    // eager single step: the scalars travel by value
    MGEA_TRY(enqueue_step(h, StepCall{B, StepKind{step_form(s->top_k == 1, false, false)}, nullptr, sampler_params(*s), logits_out_dev, false}, st));
    h->host_max_len += 1;
    if (ids_out_dev)
        MGEA_CHECK_HIP(hipMemcpyAsync(ids_out_dev, h->sampled, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return MGEA_OK;
}

}  // extern "C"
