"""The premises of tests/test_gpu_bert_kernels.py and of the [CLS] attention tests in tests/test_gpu_attention_exact.py, proved on the
CPU: every closed-form attention input isolates the key set (the Case constructor's fp64 condition), the integer slabs and GEMM
operands stay exact in fp32 (and in fp16 where they go to KV pages), and the bf16 bound admits a correctly rounded fp64 LayerNorm, so
that the reference alone never fails a test."""
import numpy as np
import torch

import bert_kernels_util as B
import decode_gemm_util as U
import test_gpu_attention_exact as AX


def test_every_cls_attention_case_satisfies_the_closed_form_condition():
    """Case.__init__ asserts 16-bit-exact inputs and |closed form - fp64 softmax attention| < 1e-6; building them all is the check"""
    n = 0
    for family, kind, S, dh in AX.cls_case_list():
        cases = AX._cls_cases(family, kind, S, dh)
        assert cases and all(c.q.shape == (AX.CLS_B, 1, AX.CLS_H, dh) and c.valid.shape == (AX.CLS_B, S) for c in cases)
        assert all(c.valid.any(1).all() for c in cases), "every row of a Case needs a valid key"
        n += len(cases)
    assert n > 300, n
    # the rows the random masks promise (S beyond one block of the kernel)
    for dh, S in ((64, 129), (64, 300), (32, 257), (32, 513)):
        m, blk = AX._cls_valid("random", S, dh), AX.CLS_BLK[dh]
        assert not m[0, :blk].any() and m[0, blk], "row 0: the whole first block masked, the first valid key at blk"
        assert not m[1, 0] and m[2].sum() == 1 and m[2, S - 1]
    for seqs, dh in ((AX.CLS_PACKED, 64), (AX.CLS_PACKED_32, 32)):
        assert 8 * len(seqs) <= dh, "the poison family gives every packed sequence 8 head dimensions of its own"
        for family in AX.FAMILIES:
            qkv, exp = AX._packed_case(family, seqs, 2, dh)
            assert qkv.shape == (sum(seqs), 6 * dh) and exp.shape == (1, sum(seqs), 2, dh)


def test_integer_slabs_and_gemm_operands_are_exact_in_fp32():
    worst = 4 * 9 + 11 + 11 + B.LIFT                      # 4 slabs, bias, residual, the lifted maximum
    assert worst < 2 ** 24
    for S, M, ldp in ((4, 5, 4104), (3, 64, 2052), (3, 6, 8324)):
        p = B.int_slabs(S, M, ldp)
        assert float(p.abs().max()) <= 9 and torch.equal(p, p.round())
        assert not torch.equal(p[0], p[1]) and not torch.equal(p[:, 0], p[:, 1]) and not torch.equal(p[..., 0], p[..., 1])
    assert int(U.int_bias(8324).abs().max()) <= 11 and float(B.int_x(5, 4096).abs().max()) <= 11
    # x 1/4 for GELU: still exact sums, arguments within +-12
    assert (3 * 9 + 11) * 0.25 <= 12
    for M, N, K in B.GEMM_EXACT + B.DIRECT_SHAPES:
        a, w = U.int_a(M, K), U.int_w(N, K)
        bound = int((a.abs().double() @ w.abs().double().t()).max()) + 11
        assert bound <= 24 * K + 11 < 2 ** 24, (M, N, K)
        out = U.int_product(a, w, U.int_bias(N))
        assert torch.equal(out.float().long(), out)
    for V in B.LOGITS_V:
        for shift in (0, 1):
            P, bias, L, first = B.argmax_slabs(3, 6, V, shift)
            assert torch.equal(P, P.round()) and float(P.abs().max()) < 2 ** 13 and int(L.max()) == B.LIFT
            assert [int(L[m].argmax()) == first[m] or int((L[m] == L[m].max()).sum()) > 1 for m in range(6)] == [True] * 6
            dup = [m for m in range(6) if int((L[m] == B.LIFT).sum()) >= 2]
            assert dup, "no row with a duplicated maximum"
    # LoRA with integers: |W| <= 11, |A| <= 3, |B| <= 8, r <= 8
    assert 11 + 2 * 8 * 3 * 8 < 2 ** 24


def test_scatter_values_are_exact_in_fp16_and_the_expected_image_keeps_poison():
    from mgea import ops
    for dh in (32, 64):
        for lens in ((3, 1), None):
            for max_pages in (3, 2):
                P, bias, ctx_len, want = B.scatter_case(dh, lens, max_pages)
                full = B.slab_sum(P, 6 * dh, bias)
                assert torch.equal(full.float().half().long(), full) and int(full.abs().max()) <= 38
                assert torch.isnan(P[:, :, 6 * dh:]).all()
                n_pages = B.n_pages_for(2, max_pages)
                table = U.permuted_table(2, max_pages, n_pages)
                img = U.expected_image(ops, full.float(), 2, dh, table, ctx_len, lens, 3, n_pages, 0, 1, torch.float16)
                bits = U.int_bits(img)
                written = int((bits != U.int_bits(ops.poison(1, torch.float16))).sum())
                tokens = sum(1 for b in range(2) for t in range(3 if lens is None else lens[b]) if (ctx_len[b] + t) // 64 < max_pages)
                assert written == tokens * 2 * 2 * dh, (dh, lens, max_pages, written, tokens)
    assert (130 // 64) == 2, "row 1 writes into logical page 2: cached with 3 table pages, dropped with 2"


def _rounded_once(want):
    """fp64 -> the nearest bf16 value (8 significant bits, ties to even) in ONE rounding; through fp32 there would be two"""
    x = want.numpy()
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 1e-300))) - 7)
    r = torch.from_numpy(np.rint(x / ulp) * ulp)
    assert torch.equal(r.float().bfloat16().double(), r), "not bf16 values"
    return r


def test_bf16_bound_admits_a_correctly_rounded_reference():
    worst = 0.0
    for D in (128, 1028, 2048):
        ids, _, t = B.embed_ids(3, 7, 0)
        word, pos, ln_w, ln_b = B.embed_tables(D, 64, seed=D)
        want = B.embed_ref(ids, t, word, pos, ln_w, ln_b, 1e-12)
        assert float(want[0].abs().max()) < 8, "the DC offset must not survive the LayerNorm"
        err = (_rounded_once(want) - want).abs()
        assert bool((err <= 2.0 ** -8 * want.abs()).all()) and bool((err <= B.bf16_bound(want)).all())
        worst = max(worst, float((err / B.bf16_bound(want)).max()))
    for C, M in ((8, 17), (520, 15), (2048, 16)):
        x = (U.rnd(M, C, seed=M + C, scale=2.0) + 0.3).bfloat16()
        want = B.ln64(x, 1 + 0.1 * U.rnd(C, seed=2), 0.1 * U.rnd(C, seed=3), 1e-5)
        err = (_rounded_once(want) - want).abs()
        assert bool((err <= B.bf16_bound(want)).all())
    assert 0.5 < worst <= 1.0, worst                      # the bound is tight: a correct rounding uses most of it
    # the embedding inputs hold what the GPU test relies on
    for packed in (0, 1):
        ids, pos_ids, t = B.embed_ids(2, 64, packed, seed=2)
        assert B.DC_ROW in ids.tolist() if packed else B.DC_ROW in ids.reshape(-1).tolist()
        assert int(ids.min()) == 0 and int(ids.max()) == B.VOCAB - 1
    ids, pos_ids, t = B.embed_ids(0, 0, 1)
    assert pos_ids.tolist() == [0] + list(range(5)) + list(range(15)), "positions restart with every packed sequence"
    h, rowstat, g, be, cu, first = B.gather_inputs(5, 7, 128, 1)
    assert cu.tolist() == [0, 1, 6, 21, 23, 87] and int(torch.isnan(h).any(1).sum()) == 87 - 5
    assert float(rowstat[first, 0].abs().max()) <= 0.3 and 0.5 <= float(rowstat[first, 1].min()) and float(rowstat[first, 1].max()) <= 1.5
    assert float(h[first].abs().max()) <= 4 and 0.8 <= float(g.min()) and float(g.max()) <= 1.2
