"""Device-resident, batched form of encode / decode / repair (leoec_*_dev).

Buffers are torch uint8 CUDA(HIP) tensors used only as device memory; work
is enqueued on the current torch stream and not synchronised.  Layout of a
batch of ``n`` objects of ``size`` bytes:

* ``objs``   — ``[n, obj_stride]``: object o's data block j at byte j*bs of row o
               (the unpadded object; bytes past ``size`` are treated as zero);
* ``parity`` — ``[n, parity_stride]``: coding block i at byte i*bs of row o.
"""
import ctypes

from . import _lib
from ._lib import lib
from .api import layout  # noqa: F401  (re-exported)

torch = _lib.torch  # (None under LEOEC_NO_TORCH=1: the device API then needs explicit streams)


def _stream(stream):
    if stream is not None:
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cid(coding):
    cid = _lib.CODING_IDS.get(coding)
    if cid is None:
        raise _lib.LeoecError(_lib.E_INVALID_CODING)
    return cid


def _row_stride(t):
    if t.dtype != torch.uint8 or not t.is_cuda:
        raise ValueError("uint8 device tensor expected")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("2-D row-contiguous tensor expected")
    if t.device.index != torch.cuda.current_device():
        raise ValueError(f"tensor on {t.device}, current device is cuda:{torch.cuda.current_device()}")
    return t.stride(0)


def _rows(t, nobj, cols, what):
    """The kernels read / write `cols` bytes of each of `nobj` rows: the
    tensor must hold them (the C ABI sees only pointers and strides)."""
    if nobj < 0 or nobj > t.shape[0]:
        raise ValueError(f"{what}: nobj {nobj} outside [0, {t.shape[0]}]")
    if nobj and t.shape[1] < cols:
        raise ValueError(f"{what}: rows of {t.shape[1]} B, {cols} B needed")


def _words(t, nobj, what):
    if t.dtype != torch.int32 or not t.is_cuda or t.dim() != 1 or (
            t.numel() > 1 and t.stride(0) != 1):
        raise ValueError(f"{what}: contiguous 1-D int32 device tensor expected")
    if t.numel() < nobj:
        raise ValueError(f"{what}: {t.numel()} words, {nobj} needed")


def _int32(device, optional, required=()):
    """The int32 word tensors of a call, ``(tensor, words, name)`` each: the
    ``optional`` ones that are None allocated on ``device``, then the
    ``required`` and the ``optional`` ones checked in that order.  Returns the
    optional ones."""
    out = [torch.empty(n, dtype=torch.int32, device=device) if t is None else t
           for t, n, _ in optional]
    for t, n, what in required:
        _words(t, n, what)
    for t, (_, n, what) in zip(out, optional):
        _words(t, n, what)
    return out


def _workspace_args(workspace):
    """(pointer, bytes) of a workspace tensor, (None, 0) of none."""
    if workspace is None:
        return None, 0
    if workspace.dtype != torch.uint8 or not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace: contiguous uint8 device tensor expected")
    return workspace.data_ptr(), workspace.numel()


def _query(name, coding, params, size, nobj):
    """leoec_<name>_dev_workspace: the bytes the call wants or needs."""
    k, m, w = params
    out = ctypes.c_uint64(0)
    _lib.check(getattr(lib, f"leoec_{name}_dev_workspace")(_cid(coding), k, m, w, size, nobj,
                                                           ctypes.byref(out)))
    return out.value


def _scrub_head(nobj):
    """The 16-byte header and one index word per object of a scrub workspace."""
    return 16 + (4 * nobj + 15) // 16 * 16


def _encode_workspace(name, workspace, need, floor, device, stream, head=None):
    """The workspace of a call that encodes into it, when the caller gave none
    and the query said ``need``: the encode region capped at
    ``VERIFY_WORKSPACE_CAP`` (the batch then goes in chunks) and at least
    ``floor`` bytes, one object's, behind ``head`` bytes where the call has a
    header.  Without a header a query of 0 needs none.  The caching allocator
    orders a buffer's reuse only on the stream it knows about, so a call on an
    explicit ``stream`` is not given one."""
    if workspace is not None or (head is None and not need):
        return workspace
    if stream is not None:
        least = f", at least {floor} B" if head is None else ""
        raise ValueError(f"{name} on an explicit stream needs an explicit workspace "
                         f"({need} B for one pass{least})")
    enc = need - (head or 0)  # 0 for everything scrub() serves
    if enc:
        enc = max(min(enc, VERIFY_WORKSPACE_CAP), floor)
    return torch.empty((head or 0) + enc, dtype=torch.uint8, device=device)


def _fixed_workspace(name, workspace, need, device, stream):
    """The workspace of a call that needs exactly the query's bytes, when the
    caller gave none (and no explicit ``stream``: _encode_workspace)."""
    if workspace is None:
        if stream is not None:
            raise ValueError(f"{name} on an explicit stream needs an explicit workspace ({need} B)")
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    return workspace


def _batch(coding, params, objs, size, parity, nobj):
    """(k, m, w, nobj, block size) of a batch whose tensors hold its rows."""
    k, m, w = params
    nobj = objs.shape[0] if nobj is None else nobj
    bs, _ = layout(coding, params, size)
    _rows(objs, nobj, size, "objs")
    _rows(parity, nobj, m * bs, "parity")
    return k, m, w, nobj, bs


def encode(coding, params, objs, size, parity, nobj=None, stream=None):
    """leoec_encode_dev: coding blocks of every object of the batch."""
    k, m, w, nobj, _ = _batch(coding, params, objs, size, parity, nobj)
    _lib.check(lib.leoec_encode_dev(_cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs),
                                    size, nobj, parity.data_ptr(), _row_stride(parity),
                                    _stream(stream)))


def decode(coding, params, objs, size, parity, erased, nobj=None, stream=None):
    """leoec_decode_dev: rebuild the erased data blocks in place in ``objs``."""
    k, m, w, nobj, _ = _batch(coding, params, objs, size, parity, nobj)
    er = (ctypes.c_int * max(len(erased), 1))(*erased)
    _lib.check(lib.leoec_decode_dev(_cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs),
                                    size, nobj, parity.data_ptr(), _row_stride(parity), er,
                                    len(erased), _stream(stream)))


VERIFY_WORKSPACE_CAP = 256 << 20  # bytes verify() allocates at most (the batch then goes in chunks)


def verify_workspace(coding, params, size, nobj):
    """leoec_verify_dev_workspace: bytes of workspace verify() wants for one
    pass over the batch; 0 where the check is fused into one kernel."""
    return _query("verify", coding, params, size, nobj)


def _pass_with_workspace(name, what, coding, params, objs, size, parity, nobj, words, workspace,
                         stream):
    """verify(), locate_ws() and locate_gfw(): one int32 word per object (the
    tensor named ``what``) from a pass that encodes into a workspace."""
    k, m, w, nobj, bs = _batch(coding, params, objs, size, parity, nobj)
    words, = _int32(objs.device, [(words, nobj, what)])
    need = _query(name, coding, params, size, nobj)
    workspace = _encode_workspace(name, workspace, need, m * bs, objs.device, stream)
    ws_ptr, ws_bytes = _workspace_args(workspace)
    _lib.check(getattr(lib, f"leoec_{name}_dev")(
        _cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs), size, nobj, parity.data_ptr(),
        _row_stride(parity), words.data_ptr(), ws_ptr, ws_bytes, _stream(stream)))
    return words


def verify(coding, params, objs, size, parity, nobj=None, flags=None, workspace=None, stream=None):
    """leoec_verify_dev: one int32 flag word per object, bit i set when the
    stored coding block i differs from the encoding of the object's data
    (0: the stripe is consistent).  ``flags`` (int32, ``nobj`` words) and
    ``workspace`` (uint8) are allocated when not given; a call on an explicit
    ``stream`` that needs a workspace must be given one, because the caching
    allocator orders a buffer's reuse only on the stream it knows about."""
    return _pass_with_workspace("verify", "flags", coding, params, objs, size, parity, nobj, flags,
                                workspace, stream)


def heal(coding, params, objs, size, parity, lost, nobj=None, unhealed=None, stream=None):
    """leoec_heal_dev: rebuild in place the blocks every object has lost.
    Bit b of ``lost[o]`` (int32, ``nobj`` words) says block b of object o is
    lost: ids below k are data blocks in ``objs``, the rest coding blocks in
    ``parity``.  Returns ``unhealed`` (int32, ``nobj`` words, allocated when
    not given): 0 for a healed or clean object, ``lost[o]`` for one that
    cannot be recovered (more than m bits, or a bit at or above k + m), of
    which nothing is written."""
    k, m, w, nobj, _ = _batch(coding, params, objs, size, parity, nobj)
    unhealed, = _int32(objs.device, [(unhealed, nobj, "unhealed")], [(lost, nobj, "lost")])
    _lib.check(lib.leoec_heal_dev(_cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs), size,
                                  nobj, parity.data_ptr(), _row_stride(parity), lost.data_ptr(),
                                  unhealed.data_ptr(), _stream(stream)))
    return unhealed


def heal_rows(coding, params, mask, coef=True):
    """leoec_heal_rows (no device needed): what heal() does for one mask of
    lost ids: ``(surv, want, rows, index)`` with the k survivor ids, the lost
    ids ascending, one list of k GF(2^w) coefficients per lost id (None with
    ``coef=False``) and the mask's record in the device table (-1 where the
    configuration has none)."""
    k, m, w = params
    surv, want = (ctypes.c_int * k)(), (ctypes.c_int * max(m, 1))()
    nwant, index = ctypes.c_int(0), ctypes.c_int(-1)
    cap = m * k
    rows = (ctypes.c_uint32 * max(cap, 1))() if coef else None
    _lib.check(lib.leoec_heal_rows(_cid(coding), k, m, w, mask, surv, want, ctypes.byref(nwant),
                                   rows, cap, ctypes.byref(index)))
    n = nwant.value
    return (list(surv), list(want[:n]),
            [list(rows[r * k:(r + 1) * k]) for r in range(n)] if coef else None, index.value)


LOCATE_MANY = 0x80000000  # LEOEC_LOCATE_MANY: inconsistent, and no single block explains it


def locate(coding, params, objs, size, parity, nobj=None, lost=None, stream=None):
    """leoec_locate_dev: one int32 word per object naming its one damaged
    block: 0 for a consistent stripe, bit b (ids below k data blocks in
    ``objs``, the rest coding blocks in ``parity``) when replacing block b
    alone makes it consistent, ``LOCATE_MANY`` (as uint32) otherwise.  Returns
    ``lost`` (int32, ``nobj`` words, allocated when not given), which heal()
    takes as it is.  vandrs w = 8 and isars with k <= 16, 2 <= m <= 4."""
    k, m, w, nobj, _ = _batch(coding, params, objs, size, parity, nobj)
    lost, = _int32(objs.device, [(lost, nobj, "lost")])
    _lib.check(lib.leoec_locate_dev(_cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs), size,
                                    nobj, parity.data_ptr(), _row_stride(parity), lost.data_ptr(),
                                    _stream(stream)))
    return lost


def _ratio_rows(entry, coding, params):
    """locate_rows() and locate_wrows(): ``m - 1`` lists of k ratios."""
    k, m, w = params
    cap = max((m - 1) * k, 1)
    ratio = (ctypes.c_uint32 * cap)()
    _lib.check(getattr(lib, entry)(_cid(coding), k, m, w, ratio, cap))
    return [list(ratio[i * k:(i + 1) * k]) for i in range(m - 1)]


def locate_rows(coding, params):
    """leoec_locate_rows (no device needed): the ratios locate() tests the
    syndromes with, ``m - 1`` lists of k GF(2^8) coefficients, list i - 1
    holding C[i][j] / C[0][j] of the coding matrix C."""
    return _ratio_rows("leoec_locate_rows", coding, params)


def locate_ws_workspace(coding, params, size, nobj):
    """leoec_locate_ws_dev_workspace: bytes of workspace locate_ws() wants for
    one pass over the batch; 0 for everything locate() serves."""
    return _query("locate_ws", coding, params, size, nobj)


def locate_ws(coding, params, objs, size, parity, nobj=None, lost=None, workspace=None,
              stream=None):
    """leoec_locate_ws_dev: locate()'s words, also for cauchyrs and liberation
    (m >= 2, k + m <= 32, (m - 1) k w <= 768), which need a workspace.
    ``workspace`` (uint8) follows verify()'s rules: allocated, up to
    ``VERIFY_WORKSPACE_CAP``, when not given, and required on an explicit
    ``stream``.  Returns ``lost``, which heal() takes as it is."""
    return _pass_with_workspace("locate_ws", "lost", coding, params, objs, size, parity, nobj, lost,
                                workspace, stream)


def locate_gfw_workspace(coding, params, size, nobj):
    """leoec_locate_gfw_dev_workspace: bytes of workspace locate_gfw() wants
    for one pass over the batch; locate_ws_workspace()'s value for everything
    locate_ws() serves."""
    return _query("locate_gfw", coding, params, size, nobj)


def locate_gfw(coding, params, objs, size, parity, nobj=None, lost=None, workspace=None,
               stream=None):
    """leoec_locate_gfw_dev: locate_ws()'s words, also for the GF(2^w) word
    classes: vandrs w = 16 / 32 and vandrs / isars w = 8 with k > 16 or m > 4
    (m >= 2, k + m <= 32), which need a workspace.  ``workspace`` (uint8)
    follows verify()'s rules: allocated, up to ``VERIFY_WORKSPACE_CAP``, when
    not given, and required on an explicit ``stream``.  Returns ``lost``,
    which heal() takes as it is."""
    return _pass_with_workspace("locate_gfw", "lost", coding, params, objs, size, parity, nobj, lost,
                                workspace, stream)


def locate_wrows(coding, params):
    """leoec_locate_wrows (no device needed): the ratios locate_gfw() tests
    the syndromes of the word classes with, ``m - 1`` lists of k GF(2^w)
    coefficients, list i - 1 holding C[i][j] / C[0][j] of the coding matrix
    C."""
    return _ratio_rows("leoec_locate_wrows", coding, params)


def scrub_workspace(coding, params, size, nobj):
    """leoec_scrub_dev_workspace: bytes of workspace scrub() needs for ``nobj``
    objects (a 16-byte header and one index word per object)."""
    return _query("scrub", coding, params, size, nobj)


def _scrub(name, coding, params, objs, size, parity, nobj, report, totals, workspace, stream):
    """scrub(), scrub_ws() and scrub_gfw(): scrub()'s workspace is the query's
    bytes, the other two calls' the header and a capped encode region."""
    k, m, w, nobj, bs = _batch(coding, params, objs, size, parity, nobj)
    report, totals = _int32(objs.device, [(report, nobj, "report"), (totals, 2, "totals")])
    need = _query(name, coding, params, size, nobj)
    if name == "scrub":
        workspace = _fixed_workspace(name, workspace, need, objs.device, stream)
    else:
        workspace = _encode_workspace(name, workspace, need, m * bs, objs.device, stream,
                                      head=_scrub_head(nobj))
    ws_ptr, ws_bytes = _workspace_args(workspace)
    _lib.check(getattr(lib, f"leoec_{name}_dev")(
        _cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs), size, nobj, parity.data_ptr(),
        _row_stride(parity), report.data_ptr(), totals.data_ptr(), ws_ptr, ws_bytes, _stream(stream)))
    return report, totals


def scrub(coding, params, objs, size, parity, nobj=None, report=None, totals=None, workspace=None,
          stream=None):
    """leoec_scrub_dev: locate() then heal() in one call, without a host round
    trip and at a cost that follows the number of damaged objects.  Returns
    ``(report, totals)``: ``report`` (int32, ``nobj`` words) holds locate()'s
    words for the batch as it was, ``objs`` and ``parity`` the bytes
    ``heal(..., lost=report)`` leaves, ``totals`` (int32, 2 words) the number of
    objects named and rebuilt and the number of ``LOCATE_MANY`` objects.
    ``report``, ``totals`` and ``workspace`` (uint8, at least
    ``scrub_workspace()`` bytes) are allocated when not given; a call on an
    explicit ``stream`` must be given the workspace, for verify()'s reason.
    vandrs w = 8 and isars with k <= 16, 2 <= m <= 4."""
    return _scrub("scrub", coding, params, objs, size, parity, nobj, report, totals, workspace,
                  stream)


def scrub_ws_workspace(coding, params, size, nobj):
    """leoec_scrub_ws_dev_workspace: bytes of workspace scrub_ws() wants for one
    pass over the batch: scrub_workspace()'s for everything scrub() serves; for
    cauchyrs and liberation the header, one index word per object and the
    encode region of ``nobj`` objects."""
    return _query("scrub_ws", coding, params, size, nobj)


def scrub_ws(coding, params, objs, size, parity, nobj=None, report=None, totals=None,
             workspace=None, stream=None):
    """leoec_scrub_ws_dev: scrub(), also for cauchyrs and liberation (m >= 2,
    k + m <= 31, (m - 1) k w <= 768): locate_ws() then heal() in one call.
    Returns ``(report, totals)`` as scrub() does.  ``workspace`` (uint8) follows
    locate_ws()'s rules: allocated when not given, its encode region up to
    ``VERIFY_WORKSPACE_CAP`` (a smaller workspace than ``scrub_ws_workspace()``
    gives the same results in more chunks of objects), and required on an
    explicit ``stream``."""
    return _scrub("scrub_ws", coding, params, objs, size, parity, nobj, report, totals, workspace,
                  stream)


def _bit_rows(entry, coding, params, *which):
    """scrub_bitrows() and heal_bitrows(): the survivors and the w row lists
    of the block ``which`` names."""
    k, m, w = params
    rw = (k * w + 31) // 32
    cap = max(w * rw, 1)
    surv = (ctypes.c_int * max(k, 1))()
    rows = (ctypes.c_uint32 * cap)()
    _lib.check(getattr(lib, entry)(_cid(coding), k, m, w, *which, surv, rows, cap))
    return list(surv[:k]), [list(rows[r * rw:(r + 1) * rw]) for r in range(w)]


def _word_rows(entry, coding, params, *which):
    """scrub_wrows() and heal_wrows(): the survivors and the k coefficients of
    the block ``which`` names."""
    k, m, w = params
    surv = (ctypes.c_int * max(k, 1))()
    coef = (ctypes.c_uint32 * max(k, 1))()
    _lib.check(getattr(lib, entry)(_cid(coding), k, m, w, *which, surv, coef, max(k, 1)))
    return list(surv[:k]), list(coef[:k])


def scrub_bitrows(coding, params, block):
    """leoec_scrub_bitrows (no device needed): the map scrub_ws() rebuilds block
    ``block`` of a cauchyrs or liberation object with.  Returns ``(surv, rows)``:
    the k survivor ids (the first k ids ascending without ``block``) and w
    lists of ``ceil(k w / 32)`` words, bit ``i w + c`` of row r set iff packet c
    of block ``surv[i]`` feeds packet r of ``block``."""
    return _bit_rows("leoec_scrub_bitrows", coding, params, block)


def scrub_gfw_workspace(coding, params, size, nobj):
    """leoec_scrub_gfw_dev_workspace: bytes of workspace scrub_gfw() wants for
    one pass over the batch: scrub_ws_workspace()'s for everything scrub_ws()
    serves; for the GF(2^w) word classes the header, one index word per object
    and the encode region of ``nobj`` objects."""
    return _query("scrub_gfw", coding, params, size, nobj)


def scrub_gfw(coding, params, objs, size, parity, nobj=None, report=None, totals=None,
              workspace=None, stream=None):
    """leoec_scrub_gfw_dev: scrub_ws(), also for the GF(2^w) word classes
    (vandrs w = 16 / 32 and vandrs / isars w = 8 with k > 16 or m > 4; m >= 2,
    k + m <= 31): locate_gfw() then heal() in one call.  Returns ``(report,
    totals)`` as scrub() does.  ``workspace`` (uint8) follows scrub_ws()'s
    rules: allocated when not given, its encode region up to
    ``VERIFY_WORKSPACE_CAP`` (a smaller workspace than ``scrub_gfw_workspace()``
    gives the same results in more chunks of objects), and required on an
    explicit ``stream``."""
    return _scrub("scrub_gfw", coding, params, objs, size, parity, nobj, report, totals, workspace,
                  stream)


def scrub_wrows(coding, params, block):
    """leoec_scrub_wrows (no device needed): the map scrub_gfw() rebuilds block
    ``block`` of an object of the GF(2^w) word classes with.  Returns ``(surv,
    coef)``: the k survivor ids (the first k ids ascending without ``block``)
    and the k GF(2^w) coefficients that give ``block`` from those survivors in
    that order."""
    return _word_rows("leoec_scrub_wrows", coding, params, block)


def heal_ws_workspace(coding, params, size, nobj):
    """leoec_heal_ws_dev_workspace: bytes of workspace heal_ws() needs for
    ``nobj`` objects (a 16-byte header and one index word per object)."""
    return _query("heal_ws", coding, params, size, nobj)


def heal_ws(coding, params, objs, size, parity, lost, nobj=None, unhealed=None, totals=None,
            workspace=None, stream=None):
    """leoec_heal_ws_dev: heal()'s bytes and ``unhealed`` for every class whose
    pattern table is at most 8 MiB, without a host round trip and at a cost
    that follows the number of damaged objects.  Returns ``(unhealed,
    totals)``: ``totals`` (int32, 2 words) holds the number of objects rebuilt
    and the number of unrecoverable ones.  ``unhealed``, ``totals`` and
    ``workspace`` (uint8, at least ``heal_ws_workspace()`` bytes) are allocated
    when not given; a call on an explicit ``stream`` must be given the
    workspace, for verify()'s reason."""
    k, m, w, nobj, _ = _batch(coding, params, objs, size, parity, nobj)
    unhealed, totals = _int32(objs.device, [(unhealed, nobj, "unhealed"), (totals, 2, "totals")],
                              [(lost, nobj, "lost")])
    need = _query("heal_ws", coding, params, size, nobj)
    ws_ptr, ws_bytes = _workspace_args(
        _fixed_workspace("heal_ws", workspace, need, objs.device, stream))
    _lib.check(lib.leoec_heal_ws_dev(_cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs),
                                     size, nobj, parity.data_ptr(), _row_stride(parity),
                                     lost.data_ptr(), unhealed.data_ptr(), totals.data_ptr(),
                                     ws_ptr, ws_bytes, _stream(stream)))
    return unhealed, totals


def update(coding, params, objs, size, parity, patch, offset, length, nobj=None, stream=None):
    """leoec_update_dev: overwrite object bytes ``[offset, offset + length)`` of
    every object of the batch with ``patch`` and patch the parity to match, in
    place: parity ^= the coding blocks of (old ^ new), so a consistent stripe
    stays consistent and a damaged one keeps its syndrome.  ``patch`` is
    ``[nobj, patch_stride]``; row o starts at the 16-byte lane that holds
    ``offset``: the new value of object byte p is
    ``patch[o, offset % 16 + (p - offset)]``."""
    k, m, w, nobj, _ = _batch(coding, params, objs, size, parity, nobj)
    if offset < 0 or length < 0:
        raise ValueError("update: negative offset or length")
    _rows(patch, nobj, offset % 16 + length if length else 0, "patch")
    _lib.check(lib.leoec_update_dev(_cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs), size,
                                    nobj, parity.data_ptr(), _row_stride(parity), patch.data_ptr(),
                                    _row_stride(patch), offset, length, _stream(stream)))


def read(coding, params, objs, size, parity, erased, offset, length, out=None, nobj=None,
         stream=None):
    """leoec_read_dev: object bytes ``[offset, offset + length)`` of every object
    of a degraded batch, the bytes ``decode(..., erased)`` would leave in
    ``objs``, without rebuilding a block and without writing ``objs`` or
    ``parity``.  Returns ``out`` (``[nobj, out_stride]``, allocated as ``nobj``
    rows of ``round_up(offset % 16 + length, 16)`` bytes when not given): row o
    starts at the 16-byte lane that holds ``offset``, so object byte p is
    ``out[o, offset % 16 + (p - offset)]``; no other byte of ``out`` is
    written."""
    k, m, w, nobj, _ = _batch(coding, params, objs, size, parity, nobj)
    if offset < 0 or length < 0:
        raise ValueError("read: negative offset or length")
    lead = offset % 16
    if out is None:
        out = torch.empty((nobj, (lead + length + 15) // 16 * 16), dtype=torch.uint8,
                          device=objs.device)
    _rows(out, nobj, lead + length if length else 0, "out")
    er = (ctypes.c_int * max(len(erased), 1))(*erased)
    _lib.check(lib.leoec_read_dev(_cid(coding), k, m, w, objs.data_ptr(), _row_stride(objs), size,
                                  nobj, parity.data_ptr(), _row_stride(parity), er, len(erased),
                                  offset, length, out.data_ptr(), _row_stride(out), _stream(stream)))
    return out


def heal_bitrows(coding, params, mask, r):
    """leoec_heal_bitrows (no device needed): the map heal_ws() rebuilds the
    r-th lost id (ascending, from 0) of ``mask`` of a cauchyrs or liberation
    object with.  Returns ``(surv, rows)`` in scrub_bitrows()'s format: the k
    survivor ids (the first k intact ids ascending) and w lists of
    ``ceil(k w / 32)`` words, bit ``i w + c`` of row t set iff packet c of
    block ``surv[i]`` feeds packet t of the lost block."""
    return _bit_rows("leoec_heal_bitrows", coding, params, mask, r)


def heal_wrows(coding, params, mask, r):
    """leoec_heal_wrows (no device needed): the map heal_ws() rebuilds the r-th
    lost id (ascending, from 0) of ``mask`` with for a vandrs or isars code
    outside heal()'s one-launch family.  Returns ``(surv, coef)``: the k
    survivor ids (the first k intact ids ascending) and the k GF(2^w)
    coefficients that give the lost block from them."""
    return _word_rows("leoec_heal_wrows", coding, params, mask, r)


def locate_bitrows(coding, params):
    """leoec_locate_bitrows (no device needed): the GF(2) ratios locate_ws()
    tests the syndromes of cauchyrs and liberation with: ``m - 1`` lists of k
    lists of w row words, ``[i - 1][j][r]`` being row r of
    T[i][j] = B[i][j] B[0][j]^-1 (bit c: syndrome packet c of coding block 0
    feeds packet r of coding block i)."""
    k, m, w = params
    cap = max((m - 1) * k * w, 1)
    rows = (ctypes.c_uint32 * cap)()
    _lib.check(lib.leoec_locate_bitrows(_cid(coding), k, m, w, rows, cap))
    return [[list(rows[((i * k) + j) * w:((i * k) + j + 1) * w]) for j in range(k)]
            for i in range(m - 1)]


def repair(coding, params, blocks, block_size, repair_ids, out, nobj, stream=None):
    """leoec_repair_dev.  ``blocks``: list of k+m tensors-or-None, each
    ``[nobj, stride]`` with the block at byte 0 of every row (all the same
    row stride); ``out``: list of tensors (same shape rules), one per id."""
    k, m, w = params
    strides = {_row_stride(b) for b in blocks if b is not None}
    ostrides = {_row_stride(o) for o in out}
    if len(strides) != 1 or len(ostrides) != 1:
        raise ValueError("one row stride per side expected")
    if len(blocks) != k + m:
        raise ValueError(f"blocks: {k + m} entries (tensor or None) expected")
    for b in blocks:
        if b is not None:
            _rows(b, nobj, block_size, "block")
    for o in out:
        _rows(o, nobj, block_size, "out")
    ptrs = (ctypes.c_void_p * (k + m))(*[b.data_ptr() if b is not None else None for b in blocks])
    optrs = (ctypes.c_void_p * max(len(out), 1))(*[o.data_ptr() for o in out])
    rep = (ctypes.c_int * max(len(repair_ids), 1))(*repair_ids)
    _lib.check(lib.leoec_repair_dev(_cid(coding), k, m, w, ptrs, strides.pop(), block_size, nobj,
                                    rep, len(repair_ids), optrs, ostrides.pop(), _stream(stream)))
