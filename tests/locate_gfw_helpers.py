"""Shared pieces of the leoec_locate_gfw_dev tests (test_locate_gfw_cpu.py, no
GPU; test_device_locate_gfw.py, product library): the GF(2^w) word families, a
numpy host model of the words (the syndromes of oracle-encoded blocks viewed as
little-endian w-bit words, leoec_locate_wrows' ratios applied with products
taken from the oracle) and one device call.  The damaged batches and their
expected words are locate_helpers.expected_calls', unchanged."""
import numpy as np

import gpu_helpers as H
import locate_helpers as L
import locate_ws_helpers as W

# class (c): the two-pass GF(2^w) shapes of the edge harness (gfs_apply at both
# widths; w = 8 with k > 16: accumulating encode launches; with m > 4: two row
# groups), isars outside the fused range and an m = 2 word code
FAMILIES = [("vandrs", 10, 4, 16, 8704), ("vandrs", 6, 3, 32, 8704), ("vandrs", 20, 4, 8, 8704),
            ("vandrs", 6, 5, 8, 8704), ("isars", 17, 4, 8, 8704), ("vandrs", 4, 2, 16, 8704)]

MANY, BIT, PREFILL, SENTINELS = L.MANY, L.BIT, L.PREFILL, L.SENTINELS
family_id = L.family_id
DTYPE = {8: np.dtype("u1"), 16: np.dtype("<u2"), 32: np.dtype("<u4")}


def word_class(cls, k, m, w):
    """Class (c) of leoec_locate_gfw_dev."""
    return (cls in ("vandrs", "isars") and w in (8, 16, 32) and not L.served(cls, k, m, w)
            and m >= 2 and k + m <= 32)


def served(cls, k, m, w):
    """The configurations the header promises an answer for."""
    return W.served(cls, k, m, w) or word_class(cls, k, m, w)


# ---------------------------------------------------------------------------
# The host model.

_tables = {}


def mul_tables(oracle, c, w):
    """[w / 8, 256]: row n holds c * (x << 8 n) for every byte x, the products
    taken from the oracle; c * word is the XOR of one entry per byte."""
    if (c, w) not in _tables:
        _tables[c, w] = np.array([[oracle.gf_mul(c, x << (8 * n), w) for x in range(256)]
                                  for n in range(w // 8)], dtype=DTYPE[w])
    return _tables[c, w]


def gf_mul_words(oracle, c, words, w):
    """c * every word of a numpy array of w-bit words."""
    t = mul_tables(oracle, c, w)
    out = np.zeros_like(words)
    for n in range(w // 8):
        out ^= t[n][(words >> (8 * n)) & 0xFF]
    return out


def model_word(oracle, cfg, data, stored, ratio):
    """The word of one object.  data: its bytes as they are now; stored: its m
    coding blocks as they are now; ratio: leoec_locate_wrows' m - 1 lists.
    Candidates are the blocks consistent with every word column: coding block
    i when every other syndrome is zero everywhere, data block j when
    s_i == T[i][j] s_0 in every word, i = 1..m-1."""
    cls, k, m, w = cfg
    ref = oracle.encode(cls, k, m, w, bytes(data))
    s = [(np.frombuffer(ref[k + i], dtype=np.uint8) ^ stored[i]).view(DTYPE[w]) for i in range(m)]
    if not any(x.any() for x in s):
        return 0
    cand = [k + i for i in range(m) if not any(s[r].any() for r in range(m) if r != i)]
    for j in range(k):
        if all(np.array_equal(gf_mul_words(oracle, ratio[i - 1][j], s[0], w), s[i])
               for i in range(1, m)):
            cand.append(j)
    return 1 << cand[0] if len(cand) == 1 else MANY


def words_of(oracle, le, case, objs):
    """The model's words for damaged objects ({o: (data bytes, [m coding
    blocks])}, scrub_helpers.damaged_objects' format); others are 0."""
    cfg = (case.cls,) + tuple(case.params)
    ratio = le.device.locate_wrows(case.cls, case.params)
    return [model_word(oracle, cfg, *objs[o], ratio) if o in objs else 0 for o in range(case.n)]


def model_words(oracle, le, case, dmg):
    """The model's words of the case's n objects under a damage list."""
    objs = {}
    for where, o, pos, x in dmg:
        if o not in objs:
            objs[o] = L.object_blocks(case, o)
        data, stored = objs[o]
        if where == "objs":
            assert 0 <= pos < case.size
            data[pos] ^= x
        else:
            assert 0 <= pos < case.m * case.bs
            stored[pos // case.bs][pos % case.bs] ^= x
    return words_of(oracle, le, case, objs)


# ---------------------------------------------------------------------------
# One device call.

def run_locate_gfw(gpu, le, case, work, par, nobj=None, workspace=None):
    """locate_helpers.run_locate for device.locate_gfw: lost in a pre-filled
    [n + 2] tensor of which the call covers words 1..n.  Returns (the [n + 2]
    tensor, the n covered words, error or None): the sentinels intact and
    every byte of both arenas, guard rows included, as it was before."""
    n, g = case.n, case.guard
    work_snap, par_snap = work.clone(), par.clone()
    lost = gpu.full((n + 2,), PREFILL, dtype=gpu.int32, device="cuda")
    lost[0], lost[n + 1] = SENTINELS
    out = le.device.locate_gfw(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                               nobj=nobj, lost=lost[1:1 + n], workspace=workspace)
    gpu.cuda.synchronize()
    assert out.data_ptr() == lost[1:1 + n].data_ptr()
    got = [int(x) & 0xFFFFFFFF for x in lost.cpu().tolist()]
    ctx = f"locate_gfw {case.ident()} bs {case.bs} nobj {nobj}"
    err = None
    if (got[0], got[-1]) != SENTINELS:
        err = f"{ctx}: sentinel words {got[0]:#x}, {got[-1]:#x}"
    err = err or (H.arena_diff(gpu, work, work_snap, g, f"{ctx}: objs") or
                  H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity"))
    return lost, got[1:-1], err
