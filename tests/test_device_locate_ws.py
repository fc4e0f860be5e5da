"""leoec_locate_ws_dev on the device: the one damaged block of every object of
damaged cauchyrs and liberation batches, word for word, on the edge harness
of gpu_helpers (guarded arenas, random non-zero bytes behind every object,
every byte of every arena compared afterwards: the call writes nothing but
its words and its workspace).

Cases: the six bitmatrix families of gpu_helpers.EDGE_FAMILIES (the per-w
packet-bitsliced encode kernels, liberation's, and cauchyrs w = 17 through the
generic bit kernel) at every size of edge_sizes: whole and partial packet
tiles, a ragged last block, empty trailing blocks: the smallest shapes at
which tiles, packet edges and padding can go wrong.  Per (family, size) the
three calls of locate_helpers.expected_calls over EDGE_N = 5 objects;
test_locate_ws_cpu.py holds the expected words against the host model.  The
third call's words then go into leoec_heal_dev unchanged."""
import pytest

import gpu_helpers as H
import locate_helpers as L
import locate_ws_helpers as W


@pytest.fixture(scope="module", params=W.FAMILIES, ids=W.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


def _cases(le, oracle, family):
    cls, k, m, w, B = family
    for size in H.edge_sizes(k, w, B):
        yield H.edge_case(le, oracle, family[:4], size)


def _hex(words):
    return [hex(x) for x in words]


@pytest.mark.gpu
def test_device_locate_ws_words(gpu, le, oracle, family):
    """The exact words of the three damaged batches of every size; sentinels
    intact, every covered word overwritten, objs and parity arenas
    byte-identical to the damaged snapshots."""
    errors = []
    for case in _cases(le, oracle, family):
        for call, (dmg, want) in enumerate(L.expected_calls(case)):
            work, par = L.damaged_arenas(gpu, case, dmg)
            _, got, err = W.run_locate_ws(gpu, le, case, work, par)
            if err:
                errors.append(err)
            if got != want:
                errors.append(f"locate_ws {case.ident()} bs {case.bs} call {1 + call}: words "
                              f"{_hex(got)}, expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_ws_partial_batch(gpu, le, oracle, family):
    """nobj = n - 2 with object n - 1 damaged as well: the words of objects
    n - 2 and n - 1 keep their pre-fill."""
    errors = []
    for case in _cases(le, oracle, family):
        n = case.n
        dmg, want = L.expected_calls(case)[0]
        work, par = L.damaged_arenas(gpu, case, dmg + [("parity", n - 1, 0, L.BIT)])
        _, got, err = W.run_locate_ws(gpu, le, case, work, par, nobj=n - 2)
        want = want[:n - 2] + [L.PREFILL] * 2
        if err:
            errors.append(err)
        if got != want:
            errors.append(f"{case.ident()}: words {_hex(got)}, expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_ws_chunked_workspace(gpu, le, oracle, family):
    """A workspace of exactly m bs bytes, one object per chunk and five chunks,
    and one of 3 m bs bytes, a chunk of three objects and a ragged one of two,
    give the words of the one-pass workspace (the query's size)."""
    errors = []
    for case in _cases(le, oracle, family):
        n, m, bs = case.n, case.m, case.bs
        assert n == 5
        assert le.device.locate_ws_workspace(case.cls, case.params, case.size, n) == n * m * bs
        dmg, want = L.expected_calls(case)[2]
        work, par = L.damaged_arenas(gpu, case, dmg)
        got = []
        for nbytes in (n * m * bs, m * bs, 3 * m * bs):
            ws = gpu.full((nbytes,), 0xEE, dtype=gpu.uint8, device="cuda")
            _, words, err = W.run_locate_ws(gpu, le, case, work, par, workspace=ws)
            if err:
                errors.append(err)
            got.append(words)
        if got[0] != want or got[1] != want or got[2] != want:
            errors.append(f"{case.ident()}: one pass {_hex(got[0])}, five chunks {_hex(got[1])}, "
                          f"chunks of three and two {_hex(got[2])}, expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_round_trip_ws(gpu, le, oracle, family):
    """The third batch located, its words handed to device.heal as they are:
    objects 0 and 3 come back to the originals byte for byte (unhealed 0),
    objects 1 and 2 are untouched (unhealed == LEOEC_LOCATE_MANY), and a
    second locate_ws finds objects 0, 3 and 4 consistent."""
    errors = []
    for case in _cases(le, oracle, family):
        n, g = case.n, case.guard
        dmg, want = L.expected_calls(case)[2]
        assert want == [1 << 0, L.MANY, L.MANY, 1 << L.last_block(case), 0]
        work, par = L.damaged_arenas(gpu, case, dmg)
        lost, got, err = W.run_locate_ws(gpu, le, case, work, par)
        ctx = f"{case.ident()} bs {case.bs}"
        if err or got != want:
            errors.append(f"{ctx}: locate_ws {_hex(got)}, expected {_hex(want)} {err or ''}")
            continue
        snap, par_snap = case.dev(gpu)
        healed_objs, healed_par = work.clone(), par.clone()  # what heal must leave
        for o in (0, 3):
            healed_objs[g + o] = snap[g + o]
        unhealed = le.device.heal(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                                  lost[1:1 + n])
        gpu.cuda.synchronize()
        left = [int(x) & 0xFFFFFFFF for x in unhealed.cpu().tolist()]
        if left != [0, L.MANY, L.MANY, 0, 0]:
            errors.append(f"{ctx}: unhealed {_hex(left)}")
        err = (H.arena_diff(gpu, work, healed_objs, g, f"heal {ctx}: objs") or
               H.arena_diff(gpu, par, healed_par, 1, f"heal {ctx}: parity"))
        if err:
            errors.append(err)
        _, again, err = W.run_locate_ws(gpu, le, case, work, par)
        if err or again != [0, L.MANY, L.MANY, 0, 0]:
            errors.append(f"{ctx}: second locate_ws {_hex(again)} {err or ''}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_ws_forwards(gpu, le, oracle):
    """vandrs(10,4,8): the query is 0 and the call, with no workspace, returns
    exactly device.locate's words."""
    family = H.EDGE_FAMILIES[0]
    cls, k, m, w, B = family
    assert (cls, k, m, w) == ("vandrs", 10, 4, 8)
    for size in H.edge_sizes(k, w, B)[:2]:
        case = H.edge_case(le, oracle, family[:4], size)
        assert le.device.locate_ws_workspace(cls, case.params, size, case.n) == 0
        for dmg, want in L.expected_calls(case):
            work, par = L.damaged_arenas(gpu, case, dmg)
            _, ref, err = L.run_locate(gpu, le, case, work, par)
            assert not err, err
            _, got, err = W.run_locate_ws(gpu, le, case, work, par, workspace=None)
            assert not err, err
            assert got == ref == want, (case.ident(), _hex(got), _hex(ref), _hex(want))
