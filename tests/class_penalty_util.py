"""The class-penalty rule of include/mgea.h (mgea_row_class_penalty, step 0b) in numpy float32, for the host and the GPU tests.

host_rule is the whole contract: three separately rounded float32 operations per penalised id and NOTHING written anywhere else.
numpy's float32 scalars round every operation to float32 (IEEE, round to nearest even), which is what __fmul_rn / __fadd_rn /
__fsub_rn do on the device; a fused multiply-add would round once where this rounds twice."""
import numpy as np


def counts(hist_row, t, window, class_of, n_class):
    """n_c over the last `window` (0 = all) of hist_row[0, t): an exact integer per class; entries outside [0, vocab) and ids of
    class -1 are skipped."""
    V = len(class_of)
    lo = max(0, t - window) if window > 0 else 0
    n = np.zeros(n_class, np.int64)
    for j in range(lo, t):
        g = int(hist_row[j])
        if not 0 <= g < V:
            continue
        c = int(class_of[g])
        if c >= 0:
            n[c] += 1
    return n


def host_rule(logits, class_of, hist, row_step, done, recs):
    """logits float32 [>= B, V] -> a copy with the rule applied to rows [0, B), B = len(recs); recs: (frequency, presence, window)
    triples.  Rows behind B, finished rows, rows whose record is off, rows at t == 0, ids of class -1 and ids of classes with
    n_c == 0 come back bit for bit."""
    out = np.array(logits, dtype=np.float32, copy=True)
    class_of = np.asarray(class_of, dtype=np.int64)
    n_class = max(int(class_of.max()) + 1, 1)
    hist = np.asarray(hist)
    for b, (freq, pres, window) in enumerate(recs):
        f, p = np.float32(freq), np.float32(pres)
        t = int(row_step[b])
        if int(done[b]) != 0 or not (f != 0 or p != 0) or t == 0:
            continue
        n = counts(hist[b], t, int(window), class_of, n_class)
        nc = np.where(class_of >= 0, n[np.maximum(class_of, 0)], 0)      # per id
        m = (f * nc.astype(np.float32)).astype(np.float32)               # rounded once
        d = (m + p).astype(np.float32)                                   # rounded again
        hit = nc > 0
        out[b, hit] = (out[b, hit] - d[hit]).astype(np.float32)          # and again
    return out
