"""The premises of tests/test_gpu_attention_forms.py, proved on the CPU: every closed-form input isolates the key set (the Case
constructor's fp64 condition) at every shape the GPU tests use, the numpy restatement of the k-tiled layout is a bijection, the
split-count rule restated in the test is the launcher's, and the masks hold the rows they promise."""
import numpy as np

import test_gpu_attention_exact as AX
import test_gpu_attention_forms as AF


def test_every_dense_case_satisfies_the_closed_form_condition():
    """Case.__init__ asserts 16-bit-exact inputs and |closed form - fp64 softmax attention| < 1e-6; building them all is the check"""
    n = 0
    for family, kind, T, dh in AF.dense_case_list():
        c = AF.dense_case(family, kind, T, dh)
        assert c.q.shape == (AF.D_B, T, AF.D_H, dh) and c.valid.shape == (AF.D_B, T)
        n += 1
    assert n == 3 * 5 * 8 * 3
    for dh in AF.D_DH:
        seqs = AF.D_PACKED[dh]
        assert 8 * len(seqs) <= dh, "the poison family gives every packed sequence 8 head dimensions of its own"
        for family in AX.FAMILIES:
            qkv, exp = AX._packed_case(family, seqs, AF.D_H, dh)
            assert qkv.shape == (sum(seqs), 3 * AF.D_H * dh) and exp.shape == (1, sum(seqs), AF.D_H, dh)
        for B, T in AF.D_TILED:
            assert B * T <= 512
            for family in AX.FAMILIES:
                assert AF.tiled_case(family, B, T, dh).valid.any(1).all()
        for S in AF.NO_KEY_S:
            AX.Case("poison", np.ones((AF.D_B, S), dtype=bool), AF.D_H, dh)
    assert 70 < 128 < 140 and (2 * 200) % 64, "(3, 70): batch row 1 lies across a 64-row group boundary; (2, 200) ends in a partial group"


def test_dense_masks_hold_the_rows_they_promise():
    for T in AF.D_T:
        for kind in AF.D_KINDS:
            valid, lens, mask = AF.dense_valid(kind, T)
            assert valid.any(1).all(), f"{kind} T={T}: every row keeps at least one valid key"
            want = np.ones_like(valid)
            if lens is not None:
                want &= np.arange(T)[None, :] < lens[:, None]
            if mask is not None:
                want &= mask
            assert np.array_equal(valid, want), "the valid set is what lens and mask say together"
            assert (kind in ("prefix_lens", "both")) == (lens is not None) and (kind in ("prefix_mask", "random", "both")) == (mask is not None)
        if T > 64:
            m = AF.dense_valid("random", T)[0]
            assert not m[0, :64].any() and m[0, 64], "row 0: the whole first 64-key tile masked, the first valid key at 64"
            assert not m[1, 0] and m[2].sum() == 1 and m[2, T - 1]
            valid, lens, mask = AF.dense_valid("both", T)
            assert valid[3].sum() == 1 and valid[3, 64], "row 3: the mask leaves keys >= 64, lens leaves key 64 of those"
            assert (mask & ~valid).any(), "lens cuts valid bits off the mask"
    # the fully masked row is the only row without a valid key
    for S in AF.NO_KEY_S:
        for how in ("mask", "lens"):
            lens, mask = AF.no_key_inputs(S, how)
            valid = np.ones((AF.D_B, S), dtype=bool)
            if lens is not None:
                valid &= np.arange(S)[None, :] < lens[:, None]
            if mask is not None:
                valid &= mask
            assert valid.any(1).tolist() == [True, False, True, True]


def test_tiled_off_restatement_is_a_bijection_of_every_row_group():
    for N in (96, 192, 288):
        for M in (1, 64, 200, 210, 400, 512):
            off = AF.tiled_map(M, N)
            groups = (M + 63) // 64
            assert off.min() == 0 and off.max() < groups * 64 * N and np.unique(off).size == M * N
        off = AF.tiled_map(512, N)
        for g in range(8):
            grp = np.sort(off[64 * g:64 * g + 64].ravel())
            assert np.array_equal(grp, np.arange(64 * N) + g * 64 * N), f"N={N}: group {g} is not mapped onto its own 64 * N floats"
        # 16-byte groups stay whole: the kernels store four consecutive n with one instruction
        assert np.array_equal(off[:, 1::4], off[:, 0::4] + 1) and np.array_equal(off[:, 3::4], off[:, 0::4] + 3) and (off[:, 0::4] % 4 == 0).all()


def paged_launch_shapes():
    """(B, H, T, max_pages) of every paged launch of the GPU tests"""
    P = AF.P_H
    return ([(2, P, 1, AX.MAX_PAGES), (5, P, 1, AX.MAX_PAGES), (2, P, 3, AX.MAX_PAGES)] + [(2, P, 1, w) for w, _, _ in AF.P_WIDTHS] +
            [(AF.LOOP_B, AF.LOOP_H, 1, AF.LOOP_WIDTH)])


def test_split_rule_restated_is_the_launchers():
    from mgea import _lib, ops
    assert _lib.tune_get("attn_split") == 64
    for B, H, T, mp in paged_launch_shapes():
        assert ops.attn_split_count(B, H, T, mp) == AF.split_rule(B, H, T, mp), (B, H, T, mp)
    for B in (1, 2, 8, 9, 33, 64, 65):          # beyond the shapes in use: both caps, and the switch's own limit
        for H in (1, 2, 8):
            for mp in (1, 4, 5, 8, 9, 16, 40, 63, 64, 65, 200):
                for T in (1, 3):
                    assert ops.attn_split_count(B, H, T, mp) == AF.split_rule(B, H, T, mp), (B, H, T, mp)
    assert [AF.split_rule(2, 2, 1, w) for w in (8, 9, 16, 64)] == [2, 3, 4, 16] and AF.split_rule(8, 8, 1, 40) == 8
    assert AF.split_rule(2, 2, 3, 16) == 1 and AF.split_rule(5, 2, 1, 16) == 4
    # the scratch the op asks for: [256 items][16 splits][head_dim + 2]
    import ctypes as C
    pf, ci = C.c_int64(0), C.c_int64(0)
    assert _lib.load().mgea_op_attn_split_scratch(96, C.byref(pf), C.byref(ci)) == 0 and (pf.value, ci.value) == (256 * 16 * 98, 256)


def test_every_paged_case_builds_and_needs_what_the_tests_say():
    n = 0
    for ctx in AF.P_LAYER_CTX + [AF.P_TILED_CTX[2], AF.P_TILED_CTX[5]] + [c for c, _ in AF.P_REUSE]:
        for _, dh in AF.P_TILED_FORMS:
            for family in AX.FAMILIES:
                n += len(AX._paged_cases(family, tuple(ctx), 1, AF.P_H, dh))
    for width, ctx, nbits in AF.P_WIDTHS:
        assert max(ctx) <= 64 * width and max(ctx) <= 2 ** nbits
        for _, dh in AF.P_FORMS:
            for family in AX.FAMILIES:
                n += len(AX._paged_cases(family, ctx, 1, AF.P_H, dh, nbits))
    for _, dh in AF.P_TILED_FORMS:
        for family in AX.FAMILIES:
            n += len(AX._paged_cases(family, (65, 131), 3, AF.P_H, dh))
    assert n > 500, n
    # the scratch sequence: 4 launched, active per row as the test states
    for ctx, active in AF.P_REUSE:
        assert tuple(AF.active_splits(c, 4) for c in ctx) == active
    assert [a for _, a in AF.P_REUSE] == [(4, 1), (2, 4), (1, 1), (4, 4)]
    # widths: 9 wide, the second row exactly fills its last page; 64 wide, the edge of the sixteenth split
    assert 576 == 9 * 64 and AF.active_splits(513, 3) == 3 and AF.active_splits(3841, 16) == 16 and AF.active_splits(3840, 16) == 15
    assert AF.active_splits(65, 16) == 1
    # the loop case: 8 splits, pg_step 32; which rows send split 0 round its loop again, and what they leave on page 32
    again = [b for b, c in enumerate(AF.LOOP_CTX) if (c + 63) // 64 > 32]
    assert again == [0, 1, 2, 5, 7] and [AF.LOOP_CTX[b] - 2048 for b in (0, 5, 7)] == [1, 2, 52]
    assert AF.LOOP_B * AF.LOOP_WIDTH == 320 and max(AF.LOOP_CTX) <= 64 * AF.LOOP_WIDTH
    for family in AX.FAMILIES:
        first, rounds = None, 0
        for c in AF.loop_cases(family):               # (one round at a time: a round holds 70 MB)
            first = c if first is None else first
            rounds += 1
            assert c.q.shape == (AF.LOOP_B, 1, AF.LOOP_H, AF.LOOP_DH)
            assert np.array_equal(c.k, first.k) and np.array_equal(c.v, first.v), "K | V are the same in every round: the page image is built once"
        assert rounds > 4 if family == "pointer" else rounds == 1
