"""leoec_locate_dev on the device: the one damaged block of every object of
damaged batches, word for word, on the edge harness of gpu_helpers (guarded
arenas, random non-zero bytes behind every object, every byte of every arena
compared afterwards: the call writes nothing but its words).

Cases: the families of locate_helpers.FAMILIES (the fused configurations at
256 lanes, gf8_locate's 64-lane form, K = 16) at every size of edge_sizes
(whole tiles, a partial last tile, a ragged last block, empty trailing
blocks).  Per (family, size) three calls over EDGE_N = 5 objects
(locate_helpers.expected_calls): verify_helpers.damage's two batches (one
flipped bit in coding block 0, in coding block m-1, in the data) and one with
two damaged bytes of one block, two damaged blocks, and a whole damaged block.
test_locate_cpu.py holds the expected words against the host model.  The
third call's words then go into leoec_heal_dev unchanged."""
import pytest

import gpu_helpers as H
import locate_helpers as L


@pytest.fixture(scope="module", params=L.FAMILIES, ids=L.family_id)
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
def test_device_locate_words(gpu, le, oracle, family):
    """The exact words of the three damaged batches of every size; sentinels
    intact, every covered word overwritten, objs and parity arenas
    byte-identical to the damaged snapshots."""
    errors = []
    for case in _cases(le, oracle, family):
        for call, (dmg, want) in enumerate(L.expected_calls(case)):
            work, par = L.damaged_arenas(gpu, case, dmg)
            _, got, err = L.run_locate(gpu, le, case, work, par)
            if err:
                errors.append(err)
            if got != want:
                errors.append(f"locate {case.ident()} bs {case.bs} call {1 + call}: words {_hex(got)}, "
                              f"expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_partial_batch(gpu, le, oracle, family):
    """nobj = n - 2 with object n - 1 damaged as well: the words of objects
    n - 2 and n - 1 keep their pre-fill."""
    errors = []
    for case in _cases(le, oracle, family):
        n = case.n
        dmg, want = L.expected_calls(case)[0]
        work, par = L.damaged_arenas(gpu, case, dmg + [("parity", n - 1, 0, L.BIT)])
        _, got, err = L.run_locate(gpu, le, case, work, par, nobj=n - 2)
        want = want[:n - 2] + [L.PREFILL] * 2
        if err:
            errors.append(err)
        if got != want:
            errors.append(f"{case.ident()}: words {_hex(got)}, expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_round_trip(gpu, le, oracle, family):
    """The third batch located, its words handed to device.heal as they are:
    objects 0 and 3 come back to the originals byte for byte (unhealed 0),
    objects 1 and 2 are untouched (unhealed == LEOEC_LOCATE_MANY), and a
    second locate finds objects 0, 3 and 4 consistent."""
    errors = []
    for case in _cases(le, oracle, family):
        n, g = case.n, case.guard
        dmg, want = L.expected_calls(case)[2]
        assert want == [1 << 0, L.MANY, L.MANY, 1 << L.last_block(case), 0]
        work, par = L.damaged_arenas(gpu, case, dmg)
        lost, got, err = L.run_locate(gpu, le, case, work, par)
        ctx = f"{case.ident()} bs {case.bs}"
        if err or got != want:
            errors.append(f"{ctx}: locate {_hex(got)}, expected {_hex(want)} {err or ''}")
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
        _, again, err = L.run_locate(gpu, le, case, work, par)
        if err or again != [0, L.MANY, L.MANY, 0, 0]:
            errors.append(f"{ctx}: second locate {_hex(again)} {err or ''}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_captured(gpu, le, oracle):
    """The call is a memset and two launches on the stream: captured into a
    graph (after one plain call, which loads the code object) it replays to
    the same words, also over a batch damaged after the capture."""
    family = L.FAMILIES[0]
    cls, k, m, w, B = family
    case = H.edge_case(le, oracle, family[:4], H.edge_sizes(k, w, B)[1])
    n, g = case.n, case.guard
    calls = L.expected_calls(case)
    work, par = L.damaged_arenas(gpu, case, calls[0][0])
    _, got, err = L.run_locate(gpu, le, case, work, par)
    assert not err and got == calls[0][1], (err, _hex(got))
    lost = gpu.full((n,), L.PREFILL, dtype=gpu.int32, device="cuda")
    gpu.cuda.synchronize()
    graph = gpu.cuda.CUDAGraph()
    with gpu.cuda.graph(graph):
        le.device.locate(cls, case.params, work[g:g + n], case.size, par[1:1 + n], lost=lost)
    graph.replay()
    gpu.cuda.synchronize()
    assert [int(x) & 0xFFFFFFFF for x in lost.cpu().tolist()] == calls[0][1]
    # the same buffers holding the third batch
    work3, par3 = L.damaged_arenas(gpu, case, calls[2][0])
    work.copy_(work3)
    par.copy_(par3)
    lost.fill_(L.PREFILL)
    graph.replay()
    gpu.cuda.synchronize()
    assert [int(x) & 0xFFFFFFFF for x in lost.cpu().tolist()] == calls[2][1]
