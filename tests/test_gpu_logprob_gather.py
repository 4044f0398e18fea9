"""mgea_op_logprob_gather alone (csrc/logprob.hip): out[m] = logits[m][targets[m]] - logsumexp(logits[m]) against the fp64 log-softmax
of the same fp32 logits.  V around the 16-byte vector width and the workgroup's stride, rows of every alignment (ld > V, odd V), a
dominant logit, flat rows, a row of -inf with one finite id, negative targets; the output lies in poison that must stay untouched.

Tolerance 2e-5: the fp32 sum of V <= 8324 terms in (0, 1] in a fixed tree carries a relative error of a few 1e-7, its logarithm the
same absolute error, and the subtraction of two fp32 values below ~100 in magnitude one rounding of 4e-6 each."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V_LIST = [31, 32, 33, 500, 8324]
M_LIST = [1, 3, 64, 200]


def _logits(M, V, ld, seed):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((M, ld), float("nan"))                   # the columns behind V are never read
    x = torch.randn(M, V, generator=g) * 3.0
    x[0::4, (7 * seed) % V] = 40.0                            # a dominant logit
    if M > 1:
        x[1::4] = 0.5                                         # flat rows
    if M > 2:
        x[2::4] = float("-inf")                               # -inf except one id
        x[2::4, V // 2] = 1.25
    buf[:, :V] = x
    return buf


@pytest.mark.parametrize("V", V_LIST)
@pytest.mark.parametrize("M", M_LIST)
def test_logprob_gather_against_fp64_log_softmax(M, V):
    from mgea import ops
    for ld in (V, V + 1, V + 7):
        buf = _logits(M, V, ld, seed=M + V)
        g = torch.Generator().manual_seed(V)
        tg = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
        tg[0::4] = (7 * (M + V)) % V                          # the dominant id itself
        if M > 2:
            tg[2] = V // 2                                    # the finite id of the -inf row: log-probability 0
        if M > 3:
            tg[3::5] = -1                                     # not scored
        want = torch.log_softmax(buf[:, :V].double(), dim=-1).gather(1, tg.clamp(min=0).long()[:, None])[:, 0]
        want = torch.where(tg < 0, torch.zeros_like(want), want)
        out = ops.poison(M + 64, device="cuda")
        dev = buf.cuda()
        got = ops.logprob_gather(dev[:, :V], tg.cuda(), out=out)
        assert bool((out[M:].view(torch.int32) == ops.POISON_BITS).all()), "wrote behind out"
        got = got[:M].double().cpu()
        fin = torch.isfinite(want)
        assert torch.equal(got[~fin], want[~fin]), "a -inf log-probability must be -inf"
        err = float((got[fin] - want[fin]).abs().max())
        assert err < 2e-5, f"M={M} V={V} ld={ld}: max |out - fp64| = {err:.3e}"
        if M > 2:
            assert float(got[2]) == 0.0


def test_logprob_gather_targets_on_the_host_are_checked_and_device_targets_clamp():
    from mgea import ops
    x = torch.randn(3, 33).cuda()
    with pytest.raises(RuntimeError, match="outside the vocabulary"):
        ops.logprob_gather(x, [0, 33, 1])
    with pytest.raises(RuntimeError, match="outside the vocabulary"):
        ops.logprob_gather(x, torch.tensor([0, 40, 1]))
    got = ops.logprob_gather(x, torch.tensor([0, 40, 1]).cuda()).cpu()
    want = torch.log_softmax(x.cpu().double(), -1)
    assert abs(float(got[1]) - float(want[1, 32])) < 2e-5          # clamped to V - 1
    assert abs(float(got[0]) - float(want[0, 0])) < 2e-5
