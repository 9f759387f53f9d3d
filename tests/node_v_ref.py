"""One (half tile, head) of the merged heads' backward (fused_bwd.hip) restated twice in fp64 numpy: in the form every instance but the
value-table one runs (dZ = dDyn M_h, Z, dM_h = dDyn^T Z, GV = sum_i p_ij dz_i) and in the value-table form of fused_bwdh_kernel<ML, true, true>
(y = M_h x_hat per node, U_j = sum_i p_ij dDyn_i, d x_hat = [dR | U] [B_h ; M_h] + GK, dM_h = U^T x_hat + u_pad (x) x_hat_pad, the padding
token's d x_hat = accK + u_pad M_h).  The two are the same function; tests/test_cpu_node_v.py holds them to 1e-12 and shows that either padding
term, once dropped, is seen.

Forward being differentiated, per token i of a hyperedge of k tokens in a row of L slots (n_pad = L - k padding keys, all equal to x_pad):
    r_i = B x_i + b,   s_ij = r_i . x_j / temp (j != i; the diagonal is masked: p_ii = 0),   s_i,pad = r_i . x_pad / temp,
    p = softmax over the k - 1 real keys and n_pad copies of the padding key,   z_i = sum_j p_ij x_j + n_pad p_i,pad x_pad,   dyn_i = M z_i.
"""
import numpy as np

TEMP = 8.0
D = 64


def make_inputs(seed, ks, L):
    """Random x_hat, r, dDyn [T, 64], B, M [64, 64], x_pad [64] and the hyperedges (first token, k) of one tile with rows of ``L`` slots."""
    rng = np.random.default_rng(seed)
    T = int(sum(ks))
    edges, t = [], 0
    for k in ks:
        assert 2 <= k <= L
        edges.append((t, k))
        t += k
    g = lambda *s: rng.standard_normal(s)
    return dict(xh=g(T, D), r=g(T, D) * 2.0, dd=g(T, D) * 0.1, B=g(D, D) / 8.0, M=g(D, D) / 8.0, xpad=g(D), edges=edges, L=L)


def probabilities(inp):
    """P [T, Lmax] (slot j of row i: key j of i's hyperedge, 0 on the diagonal and past k) and pp [T] (ONE padding slot's probability)."""
    xh, r, xpad, L = inp["xh"], inp["r"], inp["xpad"], inp["L"]
    P, pp = np.zeros((len(xh), L)), np.zeros(len(xh))
    for t0, k in inp["edges"]:
        n_pad = L - k
        for i in range(k):
            s = xh[t0:t0 + k] @ r[t0 + i] / TEMP
            s[i] = -np.inf                                   # masked diagonal
            sp = xpad @ r[t0 + i] / TEMP
            mx = max(s.max(), sp) if n_pad else s.max()
            e, ep = np.exp(s - mx), (np.exp(sp - mx) if n_pad else 0.0)
            den = e.sum() + n_pad * ep
            P[t0 + i, :k] = e / den
            pp[t0 + i] = ep / den
    return P, pp


def _rows(inp, P, pp, d_of, dpad_of):
    """What both forms share once d_ij and d_i,pad are known: dS, dR, GK, accK (the padding token's gradient as a key)."""
    xh, r, xpad, L = inp["xh"], inp["r"], inp["xpad"], inp["L"]
    T = len(xh)
    dS, dSp, dR, GK, accK = np.zeros((T, L)), np.zeros(T), np.zeros((T, D)), np.zeros((T, D)), np.zeros(D)
    for t0, k in inp["edges"]:
        n_pad = L - k
        for i in range(k):
            ti = t0 + i
            d = np.array([d_of(ti, t0 + j) for j in range(k)])
            dp = dpad_of(ti)
            ppf = n_pad * pp[ti]
            sig = P[ti, :k] @ d + ppf * dp
            dS[ti, :k] = P[ti, :k] * (d - sig) / TEMP
            dSp[ti] = ppf * (dp - sig) / TEMP
            dR[ti] = dS[ti, :k] @ xh[t0:t0 + k] + dSp[ti] * xpad
            accK += dSp[ti] * r[ti]
        for j in range(k):
            GK[t0 + j] = dS[t0:t0 + k, j] @ r[t0:t0 + k]
    return dS, dSp, dR, GK, accK


def backward_dz(inp):
    """The parent's form."""
    xh, dd, B, M, xpad, L = inp["xh"], inp["dd"], inp["B"], inp["M"], inp["xpad"], inp["L"]
    P, pp = probabilities(inp)
    dz = dd @ M                                              # dz_i = M^T dDyn_i
    Z, GV, accV = np.zeros_like(xh), np.zeros_like(xh), np.zeros(D)
    for t0, k in inp["edges"]:
        n_pad = L - k
        for i in range(k):
            Z[t0 + i] = P[t0 + i, :k] @ xh[t0:t0 + k] + n_pad * pp[t0 + i] * xpad
            accV += n_pad * pp[t0 + i] * dz[t0 + i]
        for j in range(k):
            GV[t0 + j] = P[t0:t0 + k, j] @ dz[t0:t0 + k]
    _, _, dR, GK, accK = _rows(inp, P, pp, lambda i, j: dz[i] @ xh[j], lambda i: dz[i] @ xpad)
    return dict(dx=dR @ B + GK + GV, dB=dR.T @ xh, dM=dd.T @ Z, db=dR.sum(0), dbdyn=dd.sum(0), dxpad=accK + accV)


def backward_v(inp, drop_rank_one=False, drop_upad_m=False):
    """The value-table form.  ``drop_*``: deliberately wrong variants without one of the two padding terms."""
    xh, dd, B, M, xpad, L = inp["xh"], inp["dd"], inp["B"], inp["M"], inp["xpad"], inp["L"]
    P, pp = probabilities(inp)
    y, ypad = xh @ M.T, M @ xpad                             # y_j = M x_hat_j: per NODE in the kernel (node_r_kernel's V role), gathered
    U, upad = np.zeros_like(xh), np.zeros(D)
    for t0, k in inp["edges"]:
        n_pad = L - k
        for i in range(k):
            upad += n_pad * pp[t0 + i] * dd[t0 + i]
        for j in range(k):
            U[t0 + j] = P[t0:t0 + k, j] @ dd[t0:t0 + k]
    _, _, dR, GK, accK = _rows(inp, P, pp, lambda i, j: dd[i] @ y[j], lambda i: dd[i] @ ypad)
    dx = np.concatenate([dR, U], axis=1) @ np.concatenate([B, M], axis=0) + GK          # one K = 128 product
    dM = U.T @ xh + (0.0 if drop_rank_one else np.outer(upad, xpad))
    dxpad = accK + (0.0 if drop_upad_m else upad @ M)
    return dict(dx=dx, dB=dR.T @ xh, dM=dM, db=dR.sum(0), dbdyn=dd.sum(0), dxpad=dxpad)


def worst(a, b):
    """max over the outputs of max|a - b| / max|b| (absolute where b is 0 everywhere), and the output's name."""
    errs = {n: float(np.abs(a[n] - b[n]).max() / (np.abs(b[n]).max() or 1.0)) for n in b}
    n = max(errs, key=errs.get)
    return errs[n], n, errs
