"""Device-resident batches at the edges of the block geometry: the contract of
include/leoec.h that bytes past `size` in an object row are read as zero and
never touched, and that decode rebuilds erased data blocks clipped to `size`.

Every kernel family takes a wave-uniform decision between a full tile
(unguarded 16-byte stores) and an edge tile from a minimum over its shards'
valid lengths (`vmin`).  Each test runs one device call inside guarded arenas
(gpu_helpers.check_decode / check_encode / check_repair): guard rows before
and after the batch, random non-zero bytes from `size` to the row stride of
every object, the oracle's coding blocks as decode's parity, and every byte
of every arena compared afterwards, bit-exact.  The object sizes
(gpu_helpers.edge_sizes) put the last data block at every raggedness the
layout allows, and the erasure sets (edge_erasures) put the ragged and the
empty blocks among the outputs with every survivor full, so that `vmin` is
small only if the launcher folds the outputs in.

Which row of gpu_helpers.EDGE_FAMILIES reaches which launcher (engine.cpp
apply(), kernels.hip, gfbit_inst.hip, gfs_inst.hip):

  vandrs(10,4,8), vandrs(4,2,8),   launch_gf8_t (kernels_impl.hpp): gf8_apply<K,R>,
  isars(10,4,8), vandrs(7,3,8)       256 lanes; decode of 1-4 blocks: R = 1..4
  vandrs(10,4,8) at bs 164,992     launch_gf8_t, 64 lanes (blocks above 160 KiB)
  cauchyrs(10,4,8), (6,3,4),       launch_gfb_t (gfbit_impl.hpp): gfbit_apply<W,R>,
  (5,2,11)                           per-lane guards, no vmin (held to the same contract)
  liberation(4,2,7)                launch_lib (kernels.hip): lib_apply<7> (encode);
                                     launch(LibDecApply): libb_dec_apply<7> (decode
                                     and repair through syndromes)
  liberation(10,2,11)              launch_lib: libb_apply<11> (encode, w >= 11);
                                     launch(LibDecApply): libb_dec_apply<11>
  vandrs(10,4,16), vandrs(6,3,32)  launch_gfs_t (gfs_inst.hip): gfs_apply<16|32,R>
  cauchyrs(5,3,17)                 launch(BitApply) (kernels.hip): bit_apply, the masked
                                     bitmatrix kernel (w > 16), per-packet valid lengths,
                                     no vmin (held to the same contract)

launch_gfbk_t (gfbit_impl.hpp: cauchyrs(10,4,8) launches of 4 GB and more) is
reached at these sizes only in the measurement build:
test_measure_forms.py::test_gfbk_ragged_outputs; the product's own dispatch
onto it is pinned by test_gpu_parity.py::test_cauchy_large_launch_gfbk.
"""
import pytest

import gpu_helpers as H


@pytest.fixture(scope="module", params=H.EDGE_FAMILIES, ids=lambda f: "%s-%d-%d-%d-B%d" % f)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


def _layout_rows(le, fam):
    cls, k, m, w, B = fam
    rows = []
    for size in H.edge_sizes(k, w, B):
        bs, _ = le.layout(cls, (k, m, w), size)
        rows.append((size, bs, H.block_valids(k, bs, size)))
    return rows


def test_edge_case_table(le, family):
    """The case table through the library's own layout (no GPU): every family's
    sizes really hold a whole last block, one that is no multiple of 16, one
    shorter than a 16-byte lane, an empty one, and two trailing blocks that
    are not full; the large sizes really have the block size they aim at; the
    erasure sets erase the last m data blocks and the last one alone."""
    cls, k, m, w, B = family
    rows = _layout_rows(le, family)
    last = [(bs, v[-1]) for _, bs, v in rows]
    assert any(v == bs for bs, v in last)
    assert any(v % 16 for bs, v in last)
    assert any(0 < v < 16 for bs, v in last)
    assert any(v == 0 for bs, v in last)
    assert any(v[-1] < bs and v[-2] < bs for _, bs, v in rows)
    assert any(0 < v[-2] < bs and v[-1] == 0 for _, bs, v in rows)
    # the large sizes: block size B (several tiles and a partial one), the
    # last block at both ends of the range the layout allows
    big = [(bs, v[-1]) for size, bs, v in rows if size > 16 * w * k]
    assert len(big) == 7 and all(bs == B for bs, _ in big)
    assert sorted(B - v for _, v in big) == sorted([0, 1, 15, 16, 17, 16 * w + 5, 16 * k * w - 1])
    assert all(vv == B for size, bs, v in rows if size > 16 * w * k for vv in v[:-1])
    sets = H.edge_erasures(k, m)
    assert list(range(k - m, k)) in sets and [k - 1] in sets and list(range(m)) in sets
    assert all(len(s) <= m for s in sets) and any(0 in s and k - 1 in s for s in sets)
    assert [k - 1, k] in H.edge_repairs(k, m)


def test_edge_case_table_gfbk_straddle(le):
    """cauchyrs(10,4,8): the lists of the product test and of
    test_gfbk_ragged_outputs hold a size at which a gfbk_apply tile that lies
    inside its packet reaches past the last block's valid bytes in packet 7
    (173,428: bs 17,408, packets of 2,176 B, v 16,756, tile 1 overshoots by
    524 B; 1,048,576: v 103,936, tile 11 overshoots by 192 B)."""
    cfg = ("cauchyrs", (10, 4, 8))

    def straddle(size, tile=1024):
        bs, _ = le.layout(*cfg, size)
        return H.gfbk_straddles(bs, H.block_valids(10, bs, size)[-1], tile)

    assert le.layout(*cfg, 173428)[0] == 17408 and straddle(173428)
    assert le.layout(*cfg, 1048576)[0] == 104960 and straddle(1048576)
    for B in (4352 * 8, 17408):
        assert any(straddle(s) for s in H.edge_sizes(10, 8, B)), B
    assert ("cauchyrs", 10, 4, 8, 4352 * 8) in H.EDGE_FAMILIES
    # the wider tiles of the measurement forms (128 and 256 lanes)
    assert straddle(173428, 2048) and not straddle(173428, 4096)
    assert all(straddle(H.GFBK_WIDE_SIZE, t) for t in (1024, 2048, 4096))


@pytest.mark.gpu
def test_device_decode_edges(gpu, le, oracle, family):
    cls, k, m, w, B = family
    errors = []
    for size in H.edge_sizes(k, w, B):
        case = H.edge_case(le, oracle, family[:4], size)
        for erased in H.edge_erasures(k, m):
            err = H.check_decode(gpu, le, case, erased)
            if err:
                errors.append(err)
    assert not errors, "\n".join(errors)


@pytest.mark.gpu
def test_device_encode_edges(gpu, le, oracle, family):
    cls, k, m, w, B = family
    errors = []
    for size in H.edge_sizes(k, w, B):
        err = H.check_encode(gpu, le, H.edge_case(le, oracle, family[:4], size))
        if err:
            errors.append(err)
    assert not errors, "\n".join(errors)


@pytest.mark.gpu
def test_device_repair_edges(gpu, le, oracle, family):
    """(repair sees whole blocks only: one size per block size of the table)"""
    cls, k, m, w, B = family
    errors, seen = [], set()
    for size in H.edge_sizes(k, w, B):
        bs, _ = le.layout(cls, (k, m, w), size)
        if bs in seen:
            continue
        seen.add(bs)
        case = H.edge_case(le, oracle, family[:4], size)
        for lost in H.edge_repairs(k, m):
            err = H.check_repair(gpu, le, case, lost)
            if err:
                errors.append(err)
    assert len(seen) >= 2
    assert not errors, "\n".join(errors)
