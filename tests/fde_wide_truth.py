"""Float64 restatement of the fixed dimensional encoding at width 320 (include/maxsim.h: msim_fdew_*), independent of colpali_amd.
The width is data: it is read off G and S, whose last axis `params` draws at WIDTH unless told otherwise.

For rep r with G [R, k_sim, W] and S [R, d_proj, W] drawn as below, B = 2^k_sim:
  phi_r(x) = sum_i 2^i [<G[r, i], x> > 0]                      psi_r(x) = S[r] x / sqrt(d_proj)
  entry (r * B + b) * d_proj + j = psi_r(v)[j], v = the SUM of the query tokens in bucket b (query), the MEAN of the page rows in
  bucket b (page; an empty bucket with fill_empty takes the row whose code is nearest to b in Hamming distance, lowest index on a
  tie; zeros otherwise).
"""
import numpy as np
import torch

WIDTH = 320


def params(reps, ksim, dproj, seed, width=WIDTH):
    """G, S as float64 numpy arrays: G then S from torch.Generator().manual_seed(seed), in float32."""
    g = torch.Generator().manual_seed(seed)
    G = torch.randn((reps, ksim, width), generator=g, dtype=torch.float32)
    S = torch.randint(0, 2, (reps, dproj, width), generator=g, dtype=torch.int64).to(torch.float32) * 2 - 1
    return G.double().numpy(), S.double().numpy()


def dots(X, G):
    """<G[r, i], x> for every row: [n, R, k_sim]."""
    return np.einsum("nc,rkc->nrk", np.asarray(X, dtype=np.float64), G)


def codes(X, G):
    """phi_r of every row: int [n, R]."""
    bits = dots(X, G) > 0
    return (bits * (1 << np.arange(G.shape[1]))).sum(axis=2).astype(np.int64)


def psi(v, S_r):
    return S_r @ v / np.sqrt(S_r.shape[0])


def nearest_row(code_col, b):
    """Index of the row whose code has the smallest Hamming distance to b; the lowest index on a tie."""
    best, best_d = 0, None
    for i, code in enumerate(code_col):
        d = bin(int(code) ^ int(b)).count("1")
        if best_d is None or d < best_d:          # strict: an equal distance keeps the earlier row
            best, best_d = i, d
    return best


def bucket_vectors(X, phi_r, B, *, doc, fill_empty=True):
    """v_b [B, W] of one rep and whether bucket b holds anything [B] (float64; X [n, W], n >= 1)."""
    W = X.shape[1]
    V, used = np.zeros((B, W)), np.zeros(B, dtype=bool)
    for b in range(B):
        sel = phi_r == b
        if sel.any():
            V[b] = X[sel].mean(axis=0) if doc else X[sel].sum(axis=0)
        elif doc and fill_empty:
            V[b] = X[nearest_row(phi_r, b)]
        else:
            continue
        used[b] = True
    return V, used


def encode(X, G, S, *, doc, fill_empty=True, phi=None):
    """The encoding [F] of one page (doc=True) or query of rows X [n, W]; phi: the codes [n, R] to use (default: codes(X, G))."""
    R, ksim, W = G.shape
    X = np.asarray(X, dtype=np.float64).reshape(-1, W)
    dproj = S.shape[1]
    B = 1 << ksim
    out = np.zeros((R, B, dproj))
    if X.shape[0] == 0:
        return out.reshape(-1)
    phi = codes(X, G) if phi is None else np.asarray(phi, dtype=np.int64).reshape(X.shape[0], R)
    for r in range(R):
        V, used = bucket_vectors(X, phi[:, r], B, doc=doc, fill_empty=fill_empty)
        out[r, used] = V[used] @ S[r].T / np.sqrt(dproj)
    return out.reshape(-1)


def encode_all(rows, offsets, G, S, *, doc, fill_empty=True, phi=None):
    """Encodings [n, F] of packed items: rows [total, W], offsets [n + 1]; phi: codes [total, R] or None."""
    off = np.asarray(offsets, dtype=np.int64)
    F = G.shape[0] * (1 << G.shape[1]) * S.shape[1]
    out = np.zeros((len(off) - 1, F))
    for i in range(len(off) - 1):
        a, b = off[i], off[i + 1]
        out[i] = encode(rows[a:b], G, S, doc=doc, fill_empty=fill_empty, phi=None if phi is None else phi[a:b])
    return out
