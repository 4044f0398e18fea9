"""The truncation rule of include/mgea.h (mgea_row_truncation) restated in torch, float64 by default: temperature, top-k and top-p
through the oracle's masked_probs, then min-p, typical-p, the epsilon and the eta cutoff, in this order, each over the softmax of what
the stages before it kept.  robust() is the input condition the comparisons with the HIP sampler and with transformers' warpers use:
a row qualifies when its kept set does not depend on the arithmetic's precision or on a 1e-4 relative change of a setting or of the
logits -- a condition on the inputs, two orders above the worst fp32 accumulation error of a 14336-term sum, not a tolerance on the
code under test.  Rows that fail it are redrawn; draw_robust() fails when more than one drawn row in four is rejected."""
import math

import numpy as np
import torch

from oracle.decoder_ref import DecoderRef

STAGES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
# the settings whose redraw rate was checked on the CPU: >= 30 of 32 rows qualify with randn * 3 at V = 97 and randn * 6 at V = 8324, 14336
CASES = {"min_p": dict(min_p=0.05), "typical_lo": dict(typical_p=0.2), "typical_hi": dict(typical_p=0.9),
         "epsilon": dict(epsilon_cutoff=3e-4), "eta": dict(eta_cutoff=2e-3),
         "all": dict(min_p=0.02, typical_p=0.8, epsilon_cutoff=1e-4, eta_cutoff=1e-3)}


def logit_scale(V: int) -> float:
    return 3.0 if V < 1000 else 6.0


def _softmax_kept(lg, keep):
    return torch.softmax(torch.where(keep, lg, torch.full_like(lg, -math.inf)), -1)


def _entropy(p):
    lp = torch.where(p > 0, p.clamp_min(torch.finfo(p.dtype).tiny).log(), torch.zeros_like(p))
    return -(p * lp).sum(), lp


def _first_max(lg, keep):
    v = torch.where(keep, lg, torch.full_like(lg, -math.inf))
    return int(torch.nonzero(v == v.max()).view(-1)[0])


def truncate_row(lg, keep, min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """One row: lg the logits after the temperature division, keep the bool set top-k and top-p left.  Returns the final set."""
    keep = keep.clone()
    if min_p and min_p > 0:
        p = _softmax_kept(lg, keep)
        keep &= ~(p < min_p * p.max())
    if typical_p and 0 < typical_p < 1:
        p = _softmax_kept(lg, keep)
        H, lp = _entropy(p)
        d = torch.where(keep & (p > 0), (-lp - H).abs(), torch.full_like(p, math.inf))
        order = torch.argsort(d, stable=True)
        cum = p[order].cumsum(0)
        hit = torch.nonzero(cum >= typical_p).view(-1)
        dstar = d[order[int(hit[0])]] if len(hit) else d[keep].max()   # even all of it weighs less: the largest d
        keep &= d <= dstar
    for stage, cut in enumerate((epsilon_cutoff, eta_cutoff)):
        if not (cut and cut > 0):
            continue
        p = _softmax_kept(lg, keep)
        floor = cut
        if stage == 1:
            H, _ = _entropy(p)
            floor = min(cut, math.sqrt(cut) * math.exp(-float(H)))
        top = _first_max(lg, keep)
        out = keep & (p < floor)
        out[top] = False   # the largest remaining logit stays, the lowest id among equals
        keep &= ~out
    return keep


def truncated_probs(x, settings, temperature=1.0, top_k=None, top_p=None, dtype=torch.float64):
    """x [B, V]: the rows' processed logits (penalty, bias and bans applied).  settings: one dict of the four values for every row, or
    one (or None = all off) per row.  Returns (probs [B, V], kept bool [B, V]) in `dtype`; a top_k == 1 row ignores its settings."""
    x = torch.as_tensor(x).to(dtype)
    B = x.shape[0]
    per = [settings] * B if settings is None or isinstance(settings, dict) else list(settings)
    p0 = DecoderRef.masked_probs(x, temperature, top_k if top_k else None, top_p)
    lg = x / temperature
    keep = p0 > 0   # (entries top-k keeps that carry no mass -- banned ids -- count as not kept: they are never drawn)
    out_keep = torch.zeros_like(keep)
    probs = torch.zeros_like(p0)
    for b in range(B):
        kb = keep[b] if (per[b] is None or top_k == 1) else truncate_row(lg[b], keep[b], **per[b])
        out_keep[b] = kb
        probs[b] = _softmax_kept(lg[b], kb)
    probs = torch.where(out_keep, probs, torch.zeros_like(probs))
    return probs, out_keep & (probs > 0)


def robust(x, settings, temperature=1.0, top_k=None, top_p=None):
    """bool [B]: the rows of x whose kept set is the same in float64 and float32, with any one setting scaled by (1 +- 1e-4), and with
    the logits scaled by (1 +- 1e-4)."""
    x = torch.as_tensor(x)
    _, base = truncated_probs(x, settings, temperature, top_k, top_p)
    ok = torch.ones(x.shape[0], dtype=torch.bool)

    def same(other):
        return (other == base).all(1)

    ok &= same(truncated_probs(x.float(), settings, temperature, top_k, top_p, torch.float32)[1])
    for f in (1 - 1e-4, 1 + 1e-4):
        ok &= same(truncated_probs(x.double() * f, settings, temperature, top_k, top_p)[1])
        for name in STAGES:
            if settings.get(name):
                ok &= same(truncated_probs(x, dict(settings, **{name: settings[name] * f}), temperature, top_k, top_p)[1])
        if top_p:
            ok &= same(truncated_probs(x, settings, temperature, top_k, top_p * f)[1])
    return ok


def draw_robust(rng, B, V, settings, process=None, **sampler):
    """B rows of randn * logit_scale(V) (float32) that qualify under robust(); process (or None) maps the raw rows [B, V] to the
    processed ones robust() judges (penalty, bias: row b's own).  A row that fails is redrawn in place; more than one rejection in
    four drawn rows is an AssertionError."""
    def draw(n):
        return (rng.standard_normal((n, V)) * logit_scale(V)).astype(np.float32)

    cand = draw(B)
    drawn, rejected = B, 0
    while True:
        x = cand if process is None else process(cand)
        bad = np.nonzero(~robust(torch.from_numpy(np.asarray(x)), settings, **sampler).numpy())[0]
        if len(bad) == 0:
            return cand
        rejected += len(bad)
        drawn += len(bad)
        assert rejected * 4 <= drawn, f"robust() rejected {rejected} of {drawn} rows at V={V} {settings} {sampler}"
        cand[bad] = draw(len(bad))
