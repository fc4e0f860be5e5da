"""Shared pieces of the leoec_locate_ws_dev tests (test_locate_ws_cpu.py, no
GPU; test_device_locate_ws.py, product library): the bitmatrix families, a
numpy GF(2) model of leoec_locate_bitrows' table built from the oracle's
bitmatrices, a numpy host model of the words (the syndromes of oracle-encoded
blocks, the table applied to packets with XORs) and one device call.  The
damaged batches and their expected words are locate_helpers.expected_calls',
unchanged."""
import numpy as np

import gpu_helpers as H
import locate_helpers as L

# the six bitmatrix entries of the edge harness
FAMILIES = [f for f in H.EDGE_FAMILIES if f[0] in ("cauchyrs", "liberation")]
MAX_WORDS = 768  # (m - 1) k w at most

MANY, BIT, PREFILL, SENTINELS = L.MANY, L.BIT, L.PREFILL, L.SENTINELS
family_id = L.family_id


def served(cls, k, m, w):
    """The configurations the header promises an answer for."""
    if L.served(cls, k, m, w):
        return True
    return (cls in ("cauchyrs", "liberation") and m >= 2 and k + m <= 32 and
            (m - 1) * k * w <= MAX_WORDS)


# ---------------------------------------------------------------------------
# GF(2) arithmetic on numpy 0/1 matrices.

def oracle_bitmatrix(oracle, cls, k, m, w):
    """The (m w) x (k w) coding bitmatrix as the reference builds it."""
    if cls == "liberation":
        assert m == 2
        return oracle.liberation_coding_bitmatrix(k, w)
    return oracle.matrix_to_bitmatrix(k, m, w, oracle.cauchy_good_general_coding_matrix(k, m, w))


def gf2_rank(M):
    M = (np.array(M, dtype=np.uint8) & 1).copy()
    rank = 0
    for col in range(M.shape[1]):
        piv = [r for r in range(rank, M.shape[0]) if M[r, col]]
        if not piv:
            continue
        M[[rank, piv[0]]] = M[[piv[0], rank]]
        for r in range(M.shape[0]):
            if r != rank and M[r, col]:
                M[r] ^= M[rank]
        rank += 1
    return rank


def gf2_inv(M):
    """Inverse by Gauss-Jordan; None when singular."""
    n = M.shape[0]
    A = np.concatenate([np.array(M, dtype=np.uint8) & 1, np.eye(n, dtype=np.uint8)], axis=1)
    for col in range(n):
        piv = [r for r in range(col, n) if A[r, col]]
        if not piv:
            return None
        A[[col, piv[0]]] = A[[piv[0], col]]
        for r in range(n):
            if r != col and A[r, col]:
                A[r] ^= A[col]
    return A[:, n:]


def block(B, w, i, j):
    return B[i * w:(i + 1) * w, j * w:(j + 1) * w]


def unique(B, k, m, w):
    """The two conditions the answer's uniqueness rests on."""
    if any(gf2_rank(block(B, w, i, j)) != w for i in range(m) for j in range(k)):
        return False
    for i0 in range(m):
        for i1 in range(i0 + 1, m):
            for j0 in range(k):
                for j1 in range(j0 + 1, k):
                    minor = np.block([[block(B, w, i0, j0), block(B, w, i0, j1)],
                                      [block(B, w, i1, j0), block(B, w, i1, j1)]])
                    if gf2_rank(minor) != 2 * w:
                        return False
    return True


def rows_to_matrix(words, w):
    """w row words -> w x w 0/1 matrix, bit c of word r at [r][c]."""
    return np.array([[(x >> c) & 1 for c in range(w)] for x in words], dtype=np.uint8)


def matrix_to_rows(M):
    return [sum(int(b) << c for c, b in enumerate(row)) for row in M]


def model_rows(B, k, m, w):
    """T[i][j] = B[i][j] B[0][j]^-1 as leoec_locate_bitrows lays it out."""
    out = []
    for i in range(1, m):
        out.append([])
        for j in range(k):
            inv = gf2_inv(block(B, w, 0, j))
            assert inv is not None
            T = (block(B, w, i, j).astype(np.int64) @ inv.astype(np.int64)) & 1
            out[-1].append(matrix_to_rows(T))
    return out


# ---------------------------------------------------------------------------
# The host model of the words.

def model_word(oracle, cfg, data, stored, T):
    """The word of one object.  data: its bytes as they are now; stored: its
    m coding blocks as they are now; T: leoec_locate_bitrows' lists.
    Candidates are the blocks consistent with every bit position of a packet:
    coding block i when every other syndrome is zero everywhere, data block j
    when packet r of s_i equals the XOR of the packets c of s_0 with bit c of
    T[i][j][r] set, for every i >= 1 and r."""
    cls, k, m, w = cfg
    ref = oracle.encode(cls, k, m, w, bytes(data))
    s = [(np.frombuffer(ref[k + i], dtype=np.uint8) ^ stored[i]).reshape(w, -1) for i in range(m)]
    if not any(x.any() for x in s):
        return 0
    cand = [k + i for i in range(m) if not any(s[r].any() for r in range(m) if r != i)]
    for j in range(k):
        fits = True
        for i in range(1, m):
            for r in range(w):
                pred = np.zeros_like(s[0][0])
                for c in range(w):
                    if (T[i - 1][j][r] >> c) & 1:
                        pred ^= s[0][c]
                if not np.array_equal(pred, s[i][r]):
                    fits = False
        if fits:
            cand.append(j)
    return 1 << cand[0] if len(cand) == 1 else MANY


def model_words(oracle, le, case, dmg):
    """The model's words of the case's n objects under a damage list."""
    cfg = (case.cls,) + tuple(case.params)
    T = le.device.locate_bitrows(case.cls, case.params)
    objs = [L.object_blocks(case, o) for o in range(case.n)]
    for where, o, pos, x in dmg:
        data, stored = objs[o]
        if where == "objs":
            assert 0 <= pos < case.size
            data[pos] ^= x
        else:
            assert 0 <= pos < case.m * case.bs
            stored[pos // case.bs][pos % case.bs] ^= x
    touched = {o for _, o, _, _ in dmg}
    return [model_word(oracle, cfg, *objs[o], T) if o in touched else 0 for o in range(case.n)]


# ---------------------------------------------------------------------------
# One device call.

def run_locate_ws(gpu, le, case, work, par, nobj=None, workspace=None):
    """locate_helpers.run_locate for device.locate_ws: lost in a pre-filled
    [n + 2] tensor of which the call covers words 1..n.  Returns (the [n + 2]
    tensor, the n covered words, error or None): the sentinels intact and
    every byte of both arenas, guard rows included, as it was before."""
    n, g = case.n, case.guard
    work_snap, par_snap = work.clone(), par.clone()
    lost = gpu.full((n + 2,), PREFILL, dtype=gpu.int32, device="cuda")
    lost[0], lost[n + 1] = SENTINELS
    out = le.device.locate_ws(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                              nobj=nobj, lost=lost[1:1 + n], workspace=workspace)
    gpu.cuda.synchronize()
    assert out.data_ptr() == lost[1:1 + n].data_ptr()
    got = [int(x) & 0xFFFFFFFF for x in lost.cpu().tolist()]
    ctx = f"locate_ws {case.ident()} bs {case.bs} nobj {nobj}"
    err = None
    if (got[0], got[-1]) != SENTINELS:
        err = f"{ctx}: sentinel words {got[0]:#x}, {got[-1]:#x}"
    err = err or (H.arena_diff(gpu, work, work_snap, g, f"{ctx}: objs") or
                  H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity"))
    return lost, got[1:-1], err
