"""CTC heads in float64 numpy: the specification of csrc/ctc.hip (include/lds.h states it once more in the header's style).

Semantics
  head     z[n][v] = x_n . w_v + b_v; arg = the argmax over v, the LOWEST id among exactly equal logits; m = z[arg];
           lse = m + log sum_v exp(z_v - m).  Log-probs: z - lse.
  greedy   collapse runs of equal arg, drop blank; per emitted token: start (first frame of its run), length (run length), logprob (the mean
           of m - lse over the run).
  trellis  states 0 .. 2 L over labels l_0 .. l_{L-1}: even = blank, odd s = label (s - 1) / 2.  A path starts in state 0 or 1 and ends in
           state 2 L or 2 L - 1.  Predecessors of s: s (stay), s - 1 (step), and s - 2 (skip) when s is odd, s >= 3 and its label differs from
           the label before.  E [T][L + 1]: column 0 the blank's log-prob, column j that of label j - 1.
  score    nll = -log sum over paths = F.ctc_loss(reduction='none', zero_infinity=False); L = 0: -sum_t E[t][0]; T = 0: 0 if L = 0 else +inf.
  align    the maximum path.  Ties between predecessors: prefer stay, then step, then skip; equal final states: the blank (2 L).

A-priori bounds (derived before a kernel ran; u = 2^-24, the unit roundoff of fp32)
  1. delta_z(n, v) = (D + 2) u |x_n| |w_v| + u |b_v|.  A length-D dot product accumulated in fp32 in ANY order (fmaf chains, MFMA
     partial sums) is off by at most gamma_D sum|x_i w_i| <= D u (1 + O(D u)) |x_n| |w_v| (Cauchy-Schwarz; |.| the Euclidean norm); the
     bias add rounds once more on a value below |x||w| + |b|: one more u |x||w| and u |b|; the remaining u |x||w| covers the O(D u)^2 term
     for D <= 4096.
  2. delta_lse(n) = max_v delta_z + (V + 2 k_exp + 1) u + u (k_log log V + |lse|).
       - a shift of every logit by at most delta moves lse by at most delta (lse is 1-Lipschitz in the max norm);
       - the sum s = sum_v exp(z_v - m) of V positive terms in any order (the rescaled merges of column tiles and splits included: a
         rescale by exp(m_a - M) <= 1 is one more positive factor on terms already counted) has relative error below V u; each term
         carries k_exp ulp = at most 2 k_exp u relative; one more u for the rounding of z_v - m (|d exp| = exp |d arg|, and terms with a
         large |z_v - m| are proportionally small): relative (V + 2 k_exp + 1) u in s, which is the absolute error of log s;
       - log s itself: k_log ulp of a value <= log V;
       - the final add m + log s rounds once: u |lse|.
     k_exp = 1 and k_log = 1: the device functions the HEAD uses are HIP's expf and logf (ROCm device library, documented maximum error
     1 ulp each; no fast variants there).
  3. For emissions handed in exactly, forward and Viterbi are off by at most T (2 |A| + 16) u, A = the largest finite |alpha| of the float64
     run.  Per frame and state: alpha_t(s) = lse3(alpha_{t-1}(..)) + E.  Perturbations of the inputs pass through log-sum-exp and max with
     factor <= 1, so they ADD over frames rather than multiply.  The fresh error of a frame, with the sum taken around its maximum (whose
     own term is exactly 1): two differences d = x - m <= 0 round once each (absolute u |d| e^d <= 0.4 u in the exponential); two
     exponentials of values <= 1, each off by at most 1.4 u absolutely (the recursions use the hardware forms: exp2(d log2 e), 1 ulp on top
     of the rounded product, (1 + |d|) u e^d <= 1.4 u); two additions of a sum <= 3: 6 u -- together below 10 u absolute on a sum >= 1,
     hence <= 10 u in its log; the logarithm of a value in [1, 3] as log2(y) ln 2: <= 2 u; the add m + log(..) rounds once: u |alpha|; the
     add of E rounds once: u |alpha|.  10 + 2 < 16.  (Viterbi has only the last rounding.)
  4. Through the public entries the emissions carry delta_E = delta_z + delta_lse each, and one emission enters per frame: add T delta_E.
"""
import itertools

import numpy as np

U = 2.0 ** -24
K_EXP = 1      # HIP expf: 1 ulp
K_LOG = 1      # HIP logf: 1 ulp
NEG = -np.inf


# ---- head ----
def head_stats(X, W, b):
    """X [N, D], W [V, D], b [V] -> (z [N, V], arg [N], m [N], lse [N]) in float64"""
    z = X.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
    arg = z.argmax(axis=1)      # numpy: the first (lowest) index among equal maxima
    m = z[np.arange(len(z)), arg]
    with np.errstate(over="ignore"):
        lse = m + np.log(np.exp(z - m[:, None]).sum(axis=1))
    return z, arg, m, lse


def delta_z(X, W, b):
    """bound 1, [N, V]"""
    D = X.shape[1]
    xn = np.linalg.norm(X.astype(np.float64), axis=1)
    wn = np.linalg.norm(W.astype(np.float64), axis=1)
    return (D + 2) * U * xn[:, None] * wn[None, :] + U * np.abs(b.astype(np.float64))[None, :]


def delta_lse(X, W, b, lse):
    """bound 2, [N]"""
    V = W.shape[0]
    return delta_z(X, W, b).max(axis=1) + (V + 2 * K_EXP + 1) * U + U * (K_LOG * np.log(V) + np.abs(lse))


def top2_gap(z):
    p = np.partition(z, -2, axis=1)
    return p[:, -1] - p[:, -2]


# ---- greedy ----
def collapse(arg, blank):
    """ids of one clip -> (tokens, start, length): runs of equal ids collapsed, blank dropped"""
    arg = np.asarray(arg)
    tokens, start, length = [], [], []
    t = 0
    while t < len(arg):
        e = t
        while e < len(arg) and arg[e] == arg[t]:
            e += 1
        if arg[t] != blank:
            tokens.append(int(arg[t]))
            start.append(t)
            length.append(e - t)
        t = e
    return np.array(tokens, dtype=np.int64), np.array(start, dtype=np.int64), np.array(length, dtype=np.int64)


def greedy(arg, m, lse, blank):
    tokens, start, length = collapse(arg, blank)
    d = np.asarray(m, dtype=np.float64) - np.asarray(lse, dtype=np.float64)
    lp = np.array([d[s:s + n].mean() for s, n in zip(start, length)], dtype=np.float64)
    return tokens, start, length, lp


# ---- trellis ----
def emissions(logp, labels, blank):
    """logp [T, V], labels [L] -> E [T, L + 1] float64: the blank's column, then each label's"""
    cols = np.concatenate([[blank], np.asarray(labels, dtype=np.int64)]).astype(np.int64)
    return np.asarray(logp, dtype=np.float64)[:, cols]


def _skip_ok(labels):
    L = len(labels)
    ok = np.zeros(2 * L + 1, dtype=bool)
    for l in range(1, L):
        ok[2 * l + 1] = labels[l] != labels[l - 1]
    return ok


def _state_emission(E, S):
    """E [T, L + 1] -> [T, S]: state s reads column 0 (even) or (s + 1) / 2 (odd)"""
    cols = np.array([0 if s % 2 == 0 else (s + 1) // 2 for s in range(S)])
    return E[:, cols]


def _lse(vals):
    m = max(vals)
    if m == NEG:
        return NEG
    return m + np.log(sum(np.exp(v - m) for v in vals))


def forward(E, labels, dtype=np.float64):
    """-> (nll, A): the CTC negative log-likelihood and the largest finite |alpha| met; dtype=np.float32 runs the recursion in fp32 (the
    a-priori check of bound 3)"""
    E = np.asarray(E, dtype=dtype)
    labels = np.asarray(labels, dtype=np.int64)
    T, L = E.shape[0], len(labels)
    S = 2 * L + 1
    if T == 0:
        return (0.0 if L == 0 else np.inf), 0.0
    se = _state_emission(E, S)
    ok = _skip_ok(labels)
    a = np.full(S, NEG, dtype=dtype)
    a[0] = se[0, 0]
    if L:
        a[1] = se[0, 1]
    A = float(np.abs(a[np.isfinite(a)]).max()) if np.isfinite(a).any() else 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, T):
            x1 = np.concatenate([[NEG], a])[:S].astype(dtype)
            x2 = np.concatenate([[NEG, NEG], a])[:S].astype(dtype)
            x2 = np.where(ok, x2, NEG).astype(dtype)
            m = np.maximum(np.maximum(a, x1), x2)
            ms = np.where(np.isfinite(m), m, 0).astype(dtype)
            s = (np.exp(a - ms) + np.exp(x1 - ms)).astype(dtype) + np.exp(x2 - ms).astype(dtype)
            a = np.where(np.isfinite(m), ms + np.log(s).astype(dtype) + se[t], NEG).astype(dtype)
            fin = np.isfinite(a)
            if fin.any():
                A = max(A, float(np.abs(a[fin]).max()))
    tot = _lse([float(a[S - 1])] + ([float(a[S - 2])] if L else []))
    return (-tot if tot != NEG else np.inf), A


def viterbi(E, labels):
    """-> (score, frame_label [T] (-1 on blanks), segments [L, 2], label_logprob [L]); score = -inf and (-1, -1) segments when infeasible"""
    E = np.asarray(E, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    T, L = E.shape[0], len(labels)
    S = 2 * L + 1
    fl = np.full(T, -1, dtype=np.int64)
    seg = np.full((L, 2), -1, dtype=np.int64)
    llp = np.zeros(L, dtype=np.float64)
    if T == 0:
        return (0.0 if L == 0 else NEG), fl, seg, llp
    se = _state_emission(E, S)
    ok = _skip_ok(labels)
    a = np.full(S, NEG)
    a[0] = se[0, 0]
    if L:
        a[1] = se[0, 1]
    bp = np.zeros((T, S), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            x1 = np.concatenate([[NEG], a])[:S]
            x2 = np.where(ok, np.concatenate([[NEG, NEG], a])[:S], NEG)
            v, p = a, np.zeros(S, dtype=np.int64)
            step = x1 > v                      # strict: stay wins a tie
            v, p = np.where(step, x1, v), np.where(step, 1, p)
            skip = x2 > v                      # strict: stay and step win a tie
            v, p = np.where(skip, x2, v), np.where(skip, 2, p)
            a = np.where(v == NEG, NEG, v + se[t])
            bp[t] = p
    s = S - 1
    if L and a[S - 2] > a[S - 1]:
        s = S - 2
    score = a[s]
    if score == NEG:
        return NEG, fl, seg, llp
    for t in range(T - 1, -1, -1):
        fl[t] = (s - 1) // 2 if s % 2 else -1
        s -= bp[t, s]
    for l in range(L):
        at = np.nonzero(fl == l)[0]
        seg[l] = (at[0], at[-1] + 1)
        llp[l] = E[at, l + 1].mean()
    return float(score), fl, seg, llp


def path_states_valid(fl, L):
    """a frame_label row is a valid alignment of L labels: label indices never decrease, rise by at most one, start at <= 0 and cover 0 .. L - 1
    (blanks, -1, anywhere)"""
    lab = [int(v) for v in fl if v >= 0]
    if L == 0:
        return not lab
    if not lab or lab[0] != 0 or lab[-1] != L - 1:
        return False
    return all(0 <= b - a <= 1 for a, b in zip(lab, lab[1:]))


def path_respects_repeats(fl, labels):
    """between the frames of two adjacent EQUAL labels at least one blank"""
    fl = [int(v) for v in fl]
    for t in range(1, len(fl)):
        a, b = fl[t - 1], fl[t]
        if a >= 0 and b == a + 1 and labels[a] == labels[b]:
            return False
    return True


def path_score(E, fl):
    E = np.asarray(E, dtype=np.float64)
    return float(sum(E[t, 0 if l < 0 else l + 1] for t, l in enumerate(fl)))


def viterbi_brute(E, labels):
    """the best path score by enumerating every state sequence (T <= 6)"""
    E = np.asarray(E, dtype=np.float64)
    labels = list(labels)
    T, L = E.shape[0], len(labels)
    S = 2 * L + 1
    se = _state_emission(E, S)
    ok = _skip_ok(np.asarray(labels))
    best = NEG
    for path in itertools.product(range(S), repeat=T):
        if path[0] > 1 or path[-1] < S - 2:
            continue
        good = True
        for p, q in zip(path, path[1:]):
            d = q - p
            if d < 0 or d > 2 or (d == 2 and not ok[q]):
                good = False
                break
        if good:
            best = max(best, sum(se[t, s] for t, s in enumerate(path)))
    return best


def bound3(T, A):
    return T * (2 * abs(A) + 16) * U


def feasible(T, labels):
    labels = list(labels)
    return T >= len(labels) + sum(a == b for a, b in zip(labels, labels[1:]))


# ---- the tool's error rate ----
def edit_distance(a, b):
    """plain Levenshtein distance between two sequences"""
    a, b = list(a), list(b)
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]
