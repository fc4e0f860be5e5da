"""leoec_verify_dev on the device: per-object mismatch flags of damaged
batches, bit-exact, on the edge harness of gpu_helpers (guarded arenas,
random non-zero bytes behind every object, every byte of every arena compared
afterwards: the call writes nothing but its flag words).

Cases: every family of gpu_helpers.EDGE_FAMILIES at every size of edge_sizes
(whole tiles, a partial last tile, a ragged last block, empty trailing
blocks; the 164,992-byte vandrs row is gf8_check's 64-lane form) plus
vandrs(20,4,8) and vandrs(6,5,8), the GF(2^8) shapes outside one gf8_check
launch.  Which path serves which row (verify.hip):

  vandrs(10,4,8), (4,2,8), (7,3,8), isars(10,4,8)   gf8_check, no workspace
  everything else                                   encode plan + verify_compare

Per (family, size) two calls over EDGE_N = 5 objects (verify_helpers.damage):
one flipped bit in coding block 0, in coding block m-1, in the data, and two
clean objects; the expected word of the damaged data comes from the oracle
and must name every coding block (the codes are MDS).
"""
import pytest

import gpu_helpers as H
import verify_helpers as V


@pytest.fixture(scope="module", params=V.FAMILIES, ids=V.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


def _cases(le, oracle, family):
    cls, k, m, w, B = family
    for size in H.edge_sizes(k, w, B):
        yield H.edge_case(le, oracle, family[:4], size)


def test_expected_flags_from_oracle(le, oracle, family):
    """No GPU: for every case the oracle's re-encoding of the damaged data
    differs from the stored coding blocks in every one of them (M = 2^m - 1),
    the flips land inside the arenas, and the second call's flips sit at a
    tile start at or past the last whole tile."""
    cls, k, m, w, B = family
    for case in _cases(le, oracle, family):
        for second in (False, True):
            want = V.expected_flags(oracle, case, second)
            assert want == [1, 1 << (m - 1), (1 << m) - 1, 0, 0]
            for where, o, pos in V.damage(case, second):
                assert 0 <= o < case.n
                assert 0 <= pos < (case.size if where == "objs" else m * case.bs)
        if case.bs == B:
            p0 = V.damage(case, True)[0][2]
            tile = V.packet_tile(cls, w) or 4096
            ps = case.bs // w if V.packet_tile(cls, w) else case.bs
            q = p0 - (case.bs - ps)  # offset inside the last packet (byte kernels: the block)
            assert q % tile == 0 and 0 < q < ps and ps - q <= tile, (p0, case.bs)


def test_fused_table(le):
    """The query and the tests agree on which families need no workspace."""
    for cls, k, m, w, B in V.FAMILIES:
        need = le.device.verify_workspace(cls, (k, m, w), k * B, H.EDGE_N)
        assert (need == 0) == V.fused(cls, k, m, w), (cls, k, m, w)
        assert need in (0, H.EDGE_N * m * B)
    assert sum(V.fused(*f[:4]) for f in V.FAMILIES) == 5  # the 64-lane row included
    assert all(V.fused(*f[:4]) for f in V.GF8_FAMILIES)


@pytest.mark.gpu
def test_device_verify_flags(gpu, le, oracle, family):
    """flags == [1 << 0, 1 << (m-1), M, 0, 0] for both damaged batches of
    every size; sentinels intact, every covered word overwritten, objs and
    parity arenas byte-identical to the damaged snapshots.  Fused families
    run without a workspace, the others with the one device.verify allocates."""
    errors = []
    for case in _cases(le, oracle, family):
        errors += V.check_case(gpu, le, oracle, case)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_verify_partial_batch(gpu, le, oracle, family):
    """nobj = n - 2 with object n - 1 damaged as well: the words of objects
    n - 2 and n - 1 keep their pre-fill."""
    errors = []
    for case in _cases(le, oracle, family):
        n = case.n
        dmg = V.damage(case, False) + [("parity", n - 1, 0)]
        got, err = V.run_verify(gpu, le, case, dmg, nobj=n - 2)
        want = V.expected_flags(oracle, case, False)[:n - 2] + [V.PREFILL] * 2
        if err:
            errors.append(err)
        if got != want:
            errors.append(f"{case.ident()}: flags {[hex(x) for x in got]}, expected "
                          f"{[hex(x) for x in want]}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_verify_workspace_chunks(gpu, le, oracle, family):
    """Two-pass families: a workspace of exactly m bs bytes (one object per
    chunk) gives the flags of the full workspace, as does one of two objects
    and a half; an explicit stream without a workspace is refused.  Fused
    families: no workspace is needed, and a given one is ignored."""
    cls, k, m, w, B = family
    errors = []
    for case in _cases(le, oracle, family):
        n, bs, g = case.n, case.bs, case.guard
        need = le.device.verify_workspace(cls, (k, m, w), case.size, n)
        want = V.expected_flags(oracle, case, True)
        dmg = V.damage(case, True)
        if V.fused(cls, k, m, w):
            assert need == 0
            sizes = [None, m * bs]
        else:
            assert need == n * m * bs
            sizes = [need, m * bs, 2 * m * bs + m * bs // 2 // 16 * 16]
            snap, par_snap = case.dev(gpu)
            with pytest.raises(ValueError):
                le.device.verify(cls, (k, m, w), snap[g:g + n], case.size, par_snap[1:1 + n],
                                 stream=gpu.cuda.current_stream().cuda_stream)
        for nbytes in sizes:
            ws = None if nbytes is None else gpu.empty(nbytes, dtype=gpu.uint8, device="cuda")
            got, err = V.run_verify(gpu, le, case, dmg, workspace=ws)
            if err:
                errors.append(err)
            if got != want:
                errors.append(f"{case.ident()} workspace {nbytes}: flags {[hex(x) for x in got]}, "
                              f"expected {[hex(x) for x in want]}")
    assert not errors, "\n".join(errors[:20])
