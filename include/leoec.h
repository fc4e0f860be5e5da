/*
 * leoec.h — C ABI of the MI355X-native leo_erasure engine (libleoec.so).
 *
 * This is the drop-in seam for the reference's NIF (c_src/leo_erasure_nif.cpp).
 * The reference NIF exports gf_init/0, encode/4, decode/5, repair/5
 * (c_src/leo_erasure_nif.cpp:346-353) and implements them with C++ coder
 * classes over Jerasure / ISA-L (c_src/{rs,cauchy,liberation,irs}coding.cpp).
 * Each host entry point below is what that NIF binds once its arithmetic is
 * moved onto the GPU; the NIF keeps parsing terms and building binaries
 * (see INTEGRATION.md for the shim).  The *_dev entry points are the
 * device-resident, batched form of the same operations.
 *
 * Conventions
 *   - plain pointers and sizes only; no exceptions cross this boundary;
 *   - every function returns LEOEC_OK (0) or a negative leoec_status;
 *     leoec_strerror() gives the reference's message text for it;
 *   - reentrant and thread-safe: concurrent callers (the basho_bench t4
 *     configuration) each get their own HIP stream and staging buffers;
 *   - the GF arithmetic always runs on the GPU (HIP, gfx950); a missing or
 *     unusable device is reported as LEOEC_E_NO_DEVICE, never computed on CPU;
 *   - a call's status reflects only that call's own work.  HIP keeps one
 *     sticky last-error slot per thread (hipGetLastError /
 *     hipPeekAtLastError), shared with the caller's own HIP code:
 *       . an error pending on the calling thread before the call is never
 *         reported as the call's failure;
 *       . a call that returns LEOEC_OK and found the thread's last-error slot
 *         clean leaves it clean (a HIP failure the library recovers from is
 *         dropped from the slot);
 *       . a *_dev call in which no HIP call of its own fails leaves the
 *         caller's pending error in place: hipPeekAtLastError shows the same
 *         code before and after;
 *       . a call that fails with LEOEC_E_HIP or LEOEC_E_NOMEM may leave its
 *         own failed HIP call's code in the slot; a host-memory call that
 *         recovers from a failure clears the slot, whatever was pending.
 */
#ifndef LEOEC_H
#define LEOEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with hidden visibility; everything declared here is
 * its export table. */
#pragma GCC visibility push(default)

/* Coding classes — same numbering as CodingType (c_src/leo_erasure_nif.cpp:36-42);
 * atom names vandrs | cauchyrs | liberation | isars (nif.cpp:61-72). */
enum leoec_coding {
  LEOEC_CAUCHYRS = 1,
  LEOEC_VANDRS = 2,
  LEOEC_LIBERATION = 3,
  LEOEC_ISARS = 4,
};

enum leoec_status {
  LEOEC_OK = 0,
  LEOEC_E_INVALID_CODING = -1,      /* "Invalid Coding"                           nif.cpp:55,71   */
  LEOEC_E_PARAMS = -2,              /* "Invalid Coding Parameters"                rscoding.cpp:31 */
  LEOEC_E_PARAMS_W_RS = -3,         /* "Invalid Coding Parameters (w = 8/16/32)"  rscoding.cpp:33 */
  LEOEC_E_PARAMS_LARGER_W = -4,     /* "Invalid Coding Parameters (larger w)"     cauchycoding.cpp:34 */
  LEOEC_E_PARAMS_M2 = -5,           /* "Invalid Coding Parameters (m = 2)"        liberationcoding.cpp:31 */
  LEOEC_E_PARAMS_K_LE_W = -6,       /* "Invalid Coding Parameters (k <= w)"       liberationcoding.cpp:33 */
  LEOEC_E_PARAMS_W_PRIME = -7,      /* "Invalid Coding Parameters (w is prime)"   liberationcoding.cpp:35 */
  LEOEC_E_PARAMS_W8 = -8,           /* "Invalid Coding Parameters (w = 8)"        irscoding.cpp:36 */
  LEOEC_E_NOT_ENOUGH_BLOCKS = -9,   /* "Not Enough Blocks"                        rscoding.cpp:91 */
  LEOEC_E_NOT_UNIQUE = -10,         /* "Blocks should be unique"                  rscoding.cpp:93 */
  LEOEC_E_NON_INVERTIBLE = -11,     /* "Non Invertible"                           irscoding.cpp:203 */
  LEOEC_E_BAD_ID = -12,             /* block / repair id outside 0..k+m-1 (reference: UB) */
  LEOEC_E_BAD_SIZE = -13,           /* inconsistent block size or object size > k*bs (reference: UB) */
  LEOEC_E_UNSUPPORTED = -14,        /* parameters the field / matrix construction cannot serve */
  LEOEC_E_NOMEM = -15,              /* host or device allocation failed (reference: terminate) */
  LEOEC_E_NO_DEVICE = -16,          /* no usable gfx950 HIP device */
  LEOEC_E_HIP = -17,                /* a HIP runtime call failed */
  LEOEC_E_ARG = -18,                /* NULL pointer / negative count / misaligned device buffer */
};

/* Message text for a status (static storage). */
const char *leoec_strerror(int status);

/* ---- the NIF surface ---------------------------------------------------- */

/* gf_init/0 (c_src/leo_erasure_nif.cpp:122-128): build the GF(2^8/16/32)
 * host tables, open the HIP device and warm the caller's current device once
 * (its hardware queues, the runtime's pageable-copy staging, every kernel
 * code object, the device's batching queue, pools of streams and mapped
 * buffers for other threads' first calls: 0.2-0.4 s) so the VM's first calls
 * are not charged for them.  Idempotent; other calls open the device lazily
 * (without the warm-up). */
int leoec_gf_init(void);

/* Coder::checkParams of the class (rscoding.cpp:29-34, cauchycoding.cpp:30-35,
 * liberationcoding.cpp:29-36, irscoding.cpp:32-37; factory nif.cpp:44-72). */
int leoec_check_params(int coding, int k, int m, int w);

/* Stripe geometry (c_src/common.cpp:24-33 + rscoding.cpp:44-54):
 *   block_size = roundTo(roundTo(size, k*w) / (k*w), 16) * w
 *   filled     = number of whole blocks that alias the input (<= k)      */
int leoec_layout(int coding, int k, int m, int w, uint64_t size, uint64_t *block_size,
                 int *filled);

/* encode/4 (nif.cpp:130-166 -> RSCoding::doEncode rscoding.cpp:36-85 and the
 * other classes' doEncode).  Writes blocks filled..k+m-1 — the zero-padded tail
 * data block(s) followed by the m coding blocks — contiguously into `out`
 * ((k+m-filled)*block_size bytes), exactly the bytes of the reference's
 * freshly allocated binary; blocks 0..filled-1 are the input itself
 * (zero-copy sub-binaries in the NIF). */
int leoec_encode(int coding, int k, int m, int w, const uint8_t *obj, uint64_t size,
                 uint8_t *out, uint64_t out_size);

/* decode/5 (nif.cpp:169-249 -> doDecode, e.g. rscoding.cpp:87-154).
 * blocks[i] (block_size bytes) has id ids[i]; any order, >= k unique ids.
 * Writes the first `size` bytes of D0..Dk-1 to `out`. */
int leoec_decode(int coding, int k, int m, int w, const uint8_t *const *blocks, const int *ids,
                 int nblocks, uint64_t block_size, uint64_t size, uint8_t *out);

/* repair/5 (nif.cpp:252-344 -> doRepair, e.g. rscoding.cpp:156-211).
 * Writes the blocks repair_ids[0..nrepair-1], in that order, to
 * out + r*block_size. */
int leoec_repair(int coding, int k, int m, int w, const uint8_t *const *blocks, const int *ids,
                 int nblocks, uint64_t block_size, const int *repair_ids, int nrepair,
                 uint8_t *out);

/* ---- device-resident, batched ------------------------------------------- *
 * All pointers are HIP device pointers, 16-byte aligned, strides multiples
 * of 16; work is enqueued on `stream` (a hipStream_t, NULL = default stream)
 * and the call returns without synchronising.  `nobj` objects are processed
 * per call; object o's block j lives at base + o*stride + j*block_size.
 * Strides cover a whole row (obj_stride >= size, parity_stride >=
 * m*block_size, block/out strides >= block_size) for every nobj >= 1;
 * otherwise LEOEC_E_ARG.  The buffers themselves cannot be checked here:
 * they must hold nobj rows.
 * leoec_encode_dev, leoec_decode_dev, leoec_repair_dev, leoec_update_dev,
 * leoec_read_dev, leoec_verify_dev
 * (with and without a workspace), the three locate and the three scrub calls
 * (leoec_scrub_gfw_dev serves every class a locate call names one block for,
 * up to k + m = 31) and leoec_heal_dev where it takes one launch (see there:
 * vandrs w = 8 and isars with k <= 16, m <= 4; the other classes are healed
 * without a synchronisation through the scrub calls only)
 * allocate nothing, upload nothing and wait for nothing: every
 * memset and every launch, the several launches of a large code (k > 16,
 * m > 4) or of a chunked workspace included, goes to `stream` in order, the
 * coefficients travel as kernel arguments.  So these calls can be captured
 * into a graph, after the first call: the first call of a code on a device
 * builds its plan on the host (and heal and the scrub calls their device
 * tables, with a blocking copy) and loads the code objects it needs.       */

/* Encode nobj objects of `size` bytes each, stored at objs + o*obj_stride
 * (the unpadded object; bytes past `size` inside the last data block are
 * read as zero and never touched).  Coding block i of object o is written to
 * parity + o*parity_stride + i*block_size. */
int leoec_encode_dev(int coding, int k, int m, int w, const uint8_t *objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, uint8_t *parity, uint64_t parity_stride,
                     void *stream);

/* In-place decode: the surviving data blocks are in objs (as for encode),
 * the coding blocks in parity; the data blocks listed in erased[] are rebuilt
 * into objs (clipped to `size`).  Erased coding ids are allowed and mean
 * "not a survivor".  Survivor choice follows the reference (first k intact
 * ids ascending; isars: data survivors ascending, then coding). */
int leoec_decode_dev(int coding, int k, int m, int w, uint8_t *objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t *parity, uint64_t parity_stride,
                     const int *erased, int nerased, void *stream);

/* Generic repair: block id b of object o is at blocks[b] + o*block_stride
 * (blocks[b] == NULL: missing), each block_size bytes.  Rebuilds repair_ids
 * into out[r] + o*out_stride. */
int leoec_repair_dev(int coding, int k, int m, int w, const uint8_t *const *blocks,
                     uint64_t block_stride, uint64_t block_size, uint64_t nobj,
                     const int *repair_ids, int nrepair, uint8_t *const *out,
                     uint64_t out_stride, void *stream);

/* Workspace bytes leoec_verify_dev wants for this batch: 0 where the check is
 * fused into one kernel (vandrs w = 8 and isars with k <= 16, m <= 4);
 * otherwise nobj * m * block_size (one pass).  Needs no device. */
int leoec_verify_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                               uint64_t *bytes);

/* Check nobj stripes laid out as for leoec_encode_dev / leoec_decode_dev.
 * flags[o] (device, 4-byte aligned, nobj words, every one overwritten) gets
 * bit i set iff coding block i of object o differs from the encoding of the
 * object's data anywhere in its block_size bytes; 0 = consistent.  For
 * m > 32, bit 31 stands for every coding block >= 31.  Data bytes past
 * `size` are read as zero, as in encode.  objs and parity are never written.
 * workspace: device, 16-byte aligned; may be NULL when the query returns 0;
 * otherwise at least m * block_size bytes (one object).  A smaller workspace
 * than the query's makes the call work through the batch in chunks of
 * objects on the same stream.
 * Reading a flag word: every code here is MDS, so one damaged data block
 * changes every coding block of its encoding and sets every bit 0..m-1,
 * while one damaged coding block sets only its own bit.
 * The first verify on a device loads its own code object (1-2 ms); the
 * leoec_gf_init warm-up does not cover it. */
int leoec_verify_dev(int coding, int k, int m, int w, const uint8_t *objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t *parity, uint64_t parity_stride,
                     uint32_t *flags, void *workspace, uint64_t workspace_bytes, void *stream);

/* Rebuild, in place, the blocks each object of a batch has lost; every object
 * has its own set.  The layout is that of leoec_encode_dev / leoec_decode_dev.
 * lost and unhealed: device, 4-byte aligned, nobj words each, not aliased
 * (lost == unhealed: LEOEC_E_ARG); k + m <= 32 (else LEOEC_E_UNSUPPORTED).
 * Bit b of lost[o] (0 <= b < k+m) says block b of object o is lost: ids below
 * k are data blocks in objs, the rest coding blocks in parity.  The present
 * contents of a lost block are never read.
 * An object with at most m bits set and none at or above k+m has every lost
 * block, coding blocks included, rebuilt from its first k intact ids
 * ascending (leoec_decode_dev's survivors); data blocks are clipped to
 * `size` (bytes past it are read as zero and never touched), and unhealed[o]
 * becomes 0.  Any other object is unrecoverable: nothing of it is written and
 * unhealed[o] = lost[o].  An object with lost[o] == 0 is neither read nor
 * written.  Every word of unhealed is overwritten; lost is never written.
 * vandrs w = 8 and isars with k <= 16, m <= 4 take one launch over the whole
 * batch and never synchronise; the survivors, outputs and coefficient tables
 * of every mask of 1..m bits come from a table of the code kept on the device
 * (1.2 MB at (10,4), 8 MB at (16,4)).  The first heal of a code on a device
 * builds and uploads that table with a blocking copy (milliseconds; 6,195
 * 16 x 16 inversions at (16,4)) and loads this call's code object (1-2 ms),
 * so it belongs outside a stream capture; the leoec_gf_init warm-up covers
 * neither.  At most 16 tables are kept per process and none is ever freed;
 * a 17th (code, device) pair is served as the classes below.
 * Every other class (cauchyrs, liberation, vandrs w = 16 / 32, w = 8 with
 * k > 16 or m > 4) copies the masks back on `stream` and waits for that copy:
 * there the call synchronises the stream once and cannot be captured into a
 * graph; it then enqueues one launch per run of consecutive objects with the
 * same mask and fills unhealed from the host. */
int leoec_heal_dev(int coding, int k, int m, int w, uint8_t *objs, uint64_t obj_stride,
                   uint64_t size, uint64_t nobj, uint8_t *parity, uint64_t parity_stride,
                   const uint32_t *lost, uint32_t *unhealed, void *stream);

/* Workspace bytes leoec_heal_ws_dev needs for this batch: leoec_scrub_dev's
 * layout, 16 + round_up(4 * nobj, 16); LEOEC_E_BAD_SIZE when that overflows;
 * bytes == NULL: LEOEC_E_ARG, checked after the served checks.  Configurations
 * leoec_heal_ws_dev does not serve, and invalid ones, get its statuses.  Needs
 * no device. */
int leoec_heal_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                uint64_t *bytes);

/* leoec_heal_dev with a workspace: every class it serves rebuilt with the
 * caller's masks without a host round trip.  The result is leoec_heal_dev's
 * byte for byte: layout, alignment and stride rules, the meaning of lost, the
 * survivors (the first k intact ids ascending), the clipping of data blocks
 * to `size` (bytes past it are never touched), unhealed (0 for a healed or
 * clean object, lost[o] for one with more than m bits or a bit at or above
 * k + m, of which nothing is written; every word overwritten), lost never
 * written, lost == unhealed LEOEC_E_ARG.  An object with lost[o] == 0 is
 * untouched.  At k + m = 32 bit 31 is block 31 like any other: no word of
 * this call is LEOEC_LOCATE_MANY.
 * totals: device, 4-byte aligned, 2 words, both overwritten: totals[0] the
 * number of objects rebuilt, totals[1] the number of unrecoverable ones.
 * workspace: device, 16-byte aligned, at least leoec_heal_ws_dev_workspace's
 * bytes (a 16-byte header and one index word per object); its contents after
 * the call are unspecified.  lost, unhealed, totals or workspace NULL or
 * misaligned, unhealed, totals or lost inside the workspace, or
 * workspace_bytes below the query's: LEOEC_E_ARG.
 * Served: every class leoec_heal_dev serves (k + m <= 32, m = 1 included)
 * whose pattern table, one record per mask of 1..m lost ids, is at most
 * 8 MiB:
 *   vandrs w = 8 and isars with k <= 16, m <= 4: always (leoec_heal_dev's own
 *     table, 8 MB at (16,4));
 *   any other code: 4 * (1104 + R * (8 + m * k * c)) <= 8 * 2^20 with
 *     R = C(k+m, 1) + ... + C(k+m, m) and c = 1 for vandrs and isars, c = w
 *     for cauchyrs and liberation.  vandrs(20,4,8) (4.6 MB), cauchyrs(10,4,8)
 *     (1.9 MB) and every k + m = 32, m = 2 code are served; vandrs(16,15,8)
 *     (2^31 masks) is not.
 * Everything else is LEOEC_E_UNSUPPORTED from the call and the query,
 * returned before the device is opened: such a batch goes to leoec_heal_dev.
 * Invalid parameters keep their leoec_check_params status; nobj == 0 (and
 * size == 0, an object without blocks, as in leoec_heal_dev) is LEOEC_OK with
 * nothing written.  The checks come in the scrub calls' order: layout and
 * parameters, served, empty batch, pointers and strides, workspace, then the
 * device.
 * What runs on `stream`, per chunk of objects (a chunk only keeps a launch's
 * item count below 2^31: one chunk for any batch a device holds): a one-wave
 * launch that zeroes the list's count in the workspace's header (and, ahead
 * of the first chunk, the totals; a launch, not a memset: DESIGN.md says why),
 * one launch that writes unhealed, lists the objects to rebuild and adds to
 * the totals, and one launch of fixed size over that list that rebuilds one
 * lost block per item, so the survivors of an object are read once per lost
 * block (the fused family: once per object).  Nothing
 * is allocated, uploaded or waited for, so the call can be captured into a
 * graph, after the first call: the first call of a code builds its table on
 * the host (kept for the process's life; measured on one core of the build
 * machine's CPU for the three largest images met: 0.40 s for cauchyrs(10,4,32),
 * 7.6 MB, 1,470 inversions of 320 x 320 bit matrices; 0.12 s for vandrs(22,4,8),
 * 6.9 MB; 0.08 s for vandrs(20,4,8), 4.6 MB; a small table with large blocks
 * can take longer, liberation(29,2,29), 3.4 MB, 0.57 s for 496 inversions of
 * 841 x 841), the first call of a code on a device uploads it with a
 * blocking copy and loads the code objects (1-2 ms each); the leoec_gf_init
 * warm-up covers neither.  The table cache holds 16 tables per process and is
 * its own, beside leoec_heal_dev's (which the fused family shares with that
 * call) and the scrub calls'; past that the call counts the totals and writes
 * unhealed with one launch per chunk and then runs leoec_heal_dev's own path,
 * which synchronises the stream once.  The thread's sticky HIP error is
 * handled as by every *_dev call.
 * Cost: by the number of damaged objects, not by the batch.  Measured on an
 * MI355X, 2,048 objects of 1 MiB (Heal, "The workspace form"): a
 * clean batch 0.020 ms in every class, 0.50-0.55 of leoec_heal_dev's; 32
 * objects with two lost blocks each 0.020-0.064 ms net, 0.035-0.28 of
 * leoec_heal_dev's.  A dense batch loses to leoec_heal_dev's one launch per run
 * of equal masks, because every lost block rereads the survivors: with every
 * object damaged 1.1x for vandrs w = 8 / isars with k <= 16, m <= 4, 2.1-3.2x
 * with two lost blocks and 3.4-5.2x with four for the other classes.  A batch
 * with one common mask belongs to leoec_heal_dev / leoec_decode_dev. */
int leoec_heal_ws_dev(int coding, int k, int m, int w, uint8_t *objs, uint64_t obj_stride,
                      uint64_t size, uint64_t nobj, uint8_t *parity, uint64_t parity_stride,
                      const uint32_t *lost, uint32_t *unhealed, uint32_t *totals, void *workspace,
                      uint64_t workspace_bytes, void *stream);

/* Overwrite object bytes [offset, offset + length) of every object of a
 * stored batch with the patch, and patch the parity to match, in place.  The
 * layout, alignment and stride rules are leoec_encode_dev's; the range is in
 * object bytes and the same for every object (one range per object: nobj = 1).
 * patch: device, 16-byte aligned, patch_stride a multiple of 16 and at least
 * lead + length, lead = offset % 16.  Row o starts at the 16-byte lane that
 * holds `offset`: the new value of object byte p is
 * patch[o * patch_stride + lead + (p - offset)].  The first lead bytes of a
 * row and the bytes past lead + length are never read; patch is never written.
 * After the call, with D the object of `size` bytes that is old ^ new inside
 * the range and zero elsewhere:
 *   - objs bytes [offset, offset + length) hold the patch; every other byte of
 *     the row keeps its value, bytes past `size` included;
 *   - the parity row is the parity row before the call XOR leoec_encode_dev's
 *     coding blocks of D, byte for byte.  A stripe that was consistent is the
 *     encoding of the new object.  A stripe that was damaged keeps exactly its
 *     syndrome: update never hides corruption from a later scrub, and never
 *     repairs any;
 *   - a parity byte the encoding of D cannot reach keeps its value: for vandrs
 *     and isars every column outside the w-bit words the range touches (the
 *     16-byte lanes that hold them are rewritten with the bytes they held), for
 *     cauchyrs and liberation every packet position outside the touched ones; a
 *     coding packet whose bit-row has no set bit among the touched data packets
 *     of a position is neither read nor written there.
 * The range is split at data-block boundaries: one launch per touched data
 * block and 4 coding blocks (vandrs, isars) or 64 coding packets (cauchyrs,
 * liberation), in stream order; (3 + 2m) bytes move per patched byte.  Nothing
 * is allocated, uploaded or waited for, the coefficients travel as kernel
 * arguments, so the call can be captured into a graph after the first call of
 * a code (its host plan, this call's code object).  Serves every
 * configuration leoec_encode_dev serves, k + m > 32 included.
 * Statuses, in this order: leoec_check_params' for the layout and parameters;
 * LEOEC_OK with nothing written for nobj, length or size 0; LEOEC_E_BAD_SIZE
 * when offset + length exceeds `size` or wraps; LEOEC_E_ARG for a NULL or
 * misaligned pointer, a stride that breaks the rules above, or a patch extent
 * ((nobj - 1) * patch_stride + lead + length bytes) that overlaps the extent of
 * objs or parity (LEOEC_E_BAD_SIZE: a block of 4 GiB or more); then the
 * device.
 * Against the path without this call (a device copy of the patch into objs,
 * then leoec_encode_dev of the whole object), measured on an MI355X with
 * 2,048 objects of 1 MiB (tools/update_bench.py, profiles/update_bench.txt):
 * a 4 KiB patch takes 0.020-0.057 ms against 0.48-0.60 ms (0.03-0.11 of it), a
 * 64 KiB patch 0.31-0.73 of it, and update stops winning at a patch of about
 * 143 KB for vandrs(10,4,8), 158 KB for vandrs(10,4,16), 115 KB for
 * cauchyrs(10,4,8) and 254 KB for liberation(4,2,7): near
 * (size + m * block_size) / (1 + 2m) bytes, where the two traffic models meet.
 * A longer patch belongs to the copy and leoec_encode_dev (the whole object:
 * update takes 2.1-3.2 times as long). */
int leoec_update_dev(int coding, int k, int m, int w, uint8_t *objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, uint8_t *parity, uint64_t parity_stride,
                     const uint8_t *patch, uint64_t patch_stride, uint64_t offset,
                     uint64_t length, void *stream);

/* Read object bytes [offset, offset + length) of every object of a degraded
 * batch into `out`: the bytes leoec_decode_dev(..., erased, nerased, ...) would
 * leave in objs, byte for byte, without rebuilding a block.  objs and parity are
 * never written.  The layout, alignment and stride rules for objs and parity
 * are leoec_encode_dev's; the range is in object bytes and the same for every
 * object.
 * out has the layout of leoec_update_dev's patch: device, 16-byte aligned,
 * out_stride a multiple of 16 and at least lead + length, lead = offset % 16;
 * object byte p of object o lands at out[o * out_stride + lead + (p - offset)].
 * The first lead bytes of a row and the bytes past lead + length are never
 * written, and what out held before the call never influences the result.
 * erased[] means what it means to leoec_decode_dev: ids in 0..k+m-1, coding
 * ids allowed ("not a survivor"), the survivors the first k intact ids
 * ascending.  The present contents of an erased block, data or coding, are
 * never read.  Bytes of a survivor data block past `size` are taken as zero and
 * never dereferenced, as in encode.
 * Only what the range needs is read.  The range is split at data-block
 * boundaries:
 *   - a maximal run of intact data blocks is one launch that copies the
 *     range's own bytes (they are contiguous in the row);
 *   - an erased data block j the range meets is rebuilt for the range's bytes
 *     alone.  vandrs and isars read the 16-byte lanes that hold the range's
 *     columns in the k survivors, 16 survivors a launch.  cauchyrs and
 *     liberation read, at the lane positions the segment touches, the survivor
 *     packets whose column of block j's decode bit-rows meets a touched packet
 *     of block j, and no other survivor packet; a survivor travels as its id
 *     and its w column masks, 768 argument words a launch (768 / (w + 1)
 *     survivors).  With several launches the first stores the bytes and the
 *     later ones XOR into them, in stream order;
 *   - an erased data block the range does not meet costs nothing.
 * About (k + 1) bytes move per byte read from a lost block, 2 per byte of an
 * intact one.  Nothing is allocated, uploaded or waited for, the coefficients
 * travel as kernel arguments, so the call can be captured into a graph after
 * the first plain call of a (code, erased set, lost block): that call inverts
 * the decode map on the host (the rows are kept in a bounded host cache) and
 * loads this call's code object.  leoec_gf_init does not cover it, as it does
 * not cover leoec_update_dev's.  Serves every configuration leoec_decode_dev
 * serves, k + m > 32 included.
 * Statuses, in this order, all before the device is opened:
 * leoec_check_params' for the layout and parameters; the erased list as
 * leoec_decode_dev checks it (LEOEC_E_ARG for nerased < 0 or a NULL list with
 * nerased > 0, LEOEC_E_BAD_ID for an id outside 0..k+m-1,
 * LEOEC_E_NOT_ENOUGH_BLOCKS for fewer than k intact ids); LEOEC_OK with nothing
 * written for nobj, length or size 0; LEOEC_E_BAD_SIZE when offset + length
 * exceeds `size` or wraps; the batch checks of objs and parity (LEOEC_E_ARG;
 * LEOEC_E_BAD_SIZE: a block of 4 GiB or more), then LEOEC_E_ARG for a NULL or
 * misaligned out, an out_stride that breaks the rule above, or an out extent
 * ((nobj - 1) * out_stride + lead + length bytes) that overlaps the extent of
 * objs or parity; then the device.
 * Against the path without this call (leoec_decode_dev of the batch, then a
 * device copy of the range), measured on an MI355X with 2,048 objects of 1 MiB
 * (tools/read_bench.py, profiles/read_bench.txt): a 4 KiB range inside a lost
 * block takes 0.019-0.093 ms against 0.42-0.49 ms (0.04-0.21 of it) for
 * vandrs(10,4,8), vandrs(10,4,16), cauchyrs(10,4,8) and liberation(4,2,7).  With
 * one lost block cauchyrs and liberation win up to the whole object (0.26-0.80
 * from 64 KiB on), vandrs(10,4,8) up to about 89 KB and vandrs(10,4,16), whose
 * multiply is the bound, up to about 43 KB.  Every lost block of a range reads
 * the survivors' columns again: a range of more than about one block that meets
 * several lost blocks belongs to leoec_decode_dev and a copy (1.5-3.2 times as
 * long with m lost blocks at 256 KiB and at the whole object; liberation(4,2,7)
 * still 0.65-0.87). */
int leoec_read_dev(int coding, int k, int m, int w, const uint8_t *objs, uint64_t obj_stride,
                   uint64_t size, uint64_t nobj, const uint8_t *parity, uint64_t parity_stride,
                   const int *erased, int nerased, uint64_t offset, uint64_t length,
                   uint8_t *out, uint64_t out_stride, void *stream);

/* leoec_locate_dev's word for an object that is inconsistent in a way no
 * single block explains.  The bit lies at or above k + m, so leoec_heal_dev
 * takes the object for unrecoverable. */
#define LEOEC_LOCATE_MANY 0x80000000u

/* Name the one damaged block of every object of a batch: the step between
 * leoec_verify_dev and leoec_heal_dev.  Layout, alignment, stride rules and
 * the reading of bytes past `size` are those of leoec_verify_dev; objs and
 * parity are never written.  lost: device, 4-byte aligned, nobj words, every
 * one overwritten:
 *   0                  the stripe is consistent;
 *   one bit b < k + m  block b is the only block whose replacement makes the
 *                      stripe consistent (leoec_heal_dev's ids: below k data,
 *                      the rest coding);
 *   LEOEC_LOCATE_MANY  the stripe is inconsistent and no single block explains
 *                      it.
 * The words go into leoec_heal_dev as its `lost` as they are: a
 * LEOEC_LOCATE_MANY object is left alone and comes back in `unhealed`.
 * Served: vandrs w = 8 and isars with k <= 16 and 2 <= m <= 4.  Everything
 * else (m = 1, k > 16, m > 4, vandrs w = 16 / 32, cauchyrs, liberation) is
 * LEOEC_E_UNSUPPORTED, returned before the device is opened; invalid
 * parameters keep their leoec_check_params status; nobj == 0 is LEOEC_OK.
 * How it tells: per byte column the syndromes s_i = stored coding block i ^
 * encoding of the data are all zero (clean), non-zero in one i only (coding
 * block i), or s_i = C[i][j] / C[0][j] * s_0 for every i (data block j); an
 * object's answer is the block that fits every column.  That is unique
 * because no entry and no 2 x 2 minor of the coding matrix C is zero, which
 * every call checks (leoec_locate_rows).
 * The limit at m = 2: two parity blocks can name one damaged block or detect
 * two, not both.  With m >= 3 two damaged blocks are never taken for one
 * (LEOEC_LOCATE_MANY); with m = 2 they may be reported as a third block, and
 * healing that block then leaves a consistent but wrong stripe.
 * The call allocates nothing, uploads nothing and never synchronises: a
 * memset and two launches on `stream`, so it can be captured into a graph.
 * The first locate on a device loads its own code object (1-2 ms); the
 * leoec_gf_init warm-up does not cover it. */
int leoec_locate_dev(int coding, int k, int m, int w, const uint8_t *objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, const uint8_t *parity, uint64_t parity_stride,
                     uint32_t *lost, void *stream);

/* Workspace bytes leoec_locate_ws_dev wants for this batch: 0 for everything
 * leoec_locate_dev serves, nobj * m * block_size (one pass) for cauchyrs and
 * liberation; LEOEC_E_BAD_SIZE when that overflows; bytes == NULL:
 * LEOEC_E_ARG.  Configurations leoec_locate_ws_dev does not serve, and invalid
 * ones, get its statuses.  Needs no device. */
int leoec_locate_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                  uint64_t *bytes);

/* leoec_locate_dev with a workspace, which adds the bitmatrix classes.  Words,
 * layout, alignment, stride rules and the reading of bytes past `size` are
 * leoec_locate_dev's: every word of lost is overwritten with 0, one bit
 * b < k + m or LEOEC_LOCATE_MANY, and the words go into leoec_heal_dev as they
 * are; objs and parity are never written.  The workspace's contents after the
 * call are unspecified.
 * Served:
 *   (a) everything leoec_locate_dev serves: the call is forwarded to it, the
 *       query returns 0 and workspace may be NULL;
 *   (b) cauchyrs and liberation with m >= 2, k + m <= 32 and
 *       (m-1) * k * w <= 768 (the ratio table travels as a kernel argument).
 * Everything else (vandrs w = 16 / 32, w = 8 with k > 16 or m > 4, bitmatrix
 * m = 1, k + m > 32, a larger table such as cauchyrs(10,4,32)) is
 * LEOEC_E_UNSUPPORTED, returned before the device is opened; invalid
 * parameters keep their leoec_check_params status; nobj == 0 is LEOEC_OK.
 * workspace for (b): device, 16-byte aligned, at least m * block_size bytes
 * (one object), else LEOEC_E_ARG; a smaller workspace than the query's gives
 * the same words in more chunks of objects on the same stream.
 * How (b) tells: a block is w packets.  Per bit position of a packet, the w
 * bits the packets of syndrome s_i = stored coding block i ^ encoding of the
 * data hold there are all zero (clean), non-zero in one i only (coding block
 * i), or s_i = B[i][j] B[0][j]^-1 s_0 over GF(2) for every i (data block j),
 * B[i][j] being the w x w blocks of the coding bitmatrix; an object's answer
 * is the block that fits every position.  That is unique because every
 * B[i][j] and every 2w x 2w minor of two coding rows and two data columns is
 * invertible, which every call checks (leoec_locate_bitrows).
 * The limit at m = 2 is leoec_locate_dev's and holds for every liberation
 * call: two damaged blocks may be reported as a third.  At k + m = 32 the bit
 * of the last coding block (id 31) is LEOEC_LOCATE_MANY's own: that word says
 * either, and leoec_heal_dev reads it as block 31.
 * For (b) the call allocates nothing, uploads nothing and never synchronises:
 * per chunk the class's encode into the workspace, a memset and two launches
 * on `stream`.  The first call on a device loads its own code object (1-2 ms);
 * the leoec_gf_init warm-up does not cover it. */
int leoec_locate_ws_dev(int coding, int k, int m, int w, const uint8_t *objs, uint64_t obj_stride,
                        uint64_t size, uint64_t nobj, const uint8_t *parity, uint64_t parity_stride,
                        uint32_t *lost, void *workspace, uint64_t workspace_bytes, void *stream);

/* Workspace bytes leoec_locate_gfw_dev wants for this batch: for everything
 * leoec_locate_ws_dev serves, that call's query (same value, same statuses);
 * for class (c) below nobj * m * block_size (one pass); LEOEC_E_BAD_SIZE when
 * that overflows; bytes == NULL: LEOEC_E_ARG, checked after the served checks.
 * Configurations leoec_locate_gfw_dev does not serve, and invalid ones, get
 * its statuses.  Needs no device. */
int leoec_locate_gfw_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                   uint64_t *bytes);

/* leoec_locate_ws_dev plus the GF(2^w) word classes, in the relation
 * leoec_locate_ws_dev has to leoec_locate_dev.  Words, layout, alignment,
 * stride rules and the reading of bytes past `size` are leoec_locate_ws_dev's:
 * every word of lost is overwritten with 0, one bit b < k + m or
 * LEOEC_LOCATE_MANY, and the words go into leoec_heal_dev as they are; objs
 * and parity are never written.  The workspace's contents after the call are
 * unspecified.
 * Served:
 *   (a) everything leoec_locate_ws_dev serves (its classes (a) and (b)): the
 *       call and the query are forwarded to it, with the same statuses,
 *       workspace size and words;
 *   (c) vandrs w = 16 / 32, and vandrs / isars w = 8 with k > 16 or m > 4, all
 *       with m >= 2 and k + m <= 32 (one bit of the word per block).
 * Everything else (m = 1, k + m > 32, the bitmatrix configurations
 * leoec_locate_ws_dev refuses) is LEOEC_E_UNSUPPORTED, returned before the
 * device is opened; invalid parameters keep their leoec_check_params status;
 * nobj == 0 is LEOEC_OK with nothing written.  The checks come in
 * leoec_locate_ws_dev's order: layout and parameters, served, empty batch,
 * pointers and strides, workspace, then the device.
 * workspace for (c): device, 16-byte aligned, at least m * block_size bytes
 * (one object), else LEOEC_E_ARG; a smaller workspace than the query's gives
 * the same words in more chunks of objects on the same stream.
 * How (c) tells: a block is a row of little-endian w-bit words.  Per word
 * column the syndromes s_i = stored coding block i ^ encoding of the data are
 * all zero (clean), non-zero in one i only (coding block i), or
 * s_i = C[i][j] / C[0][j] * s_0 in GF(2^w) for every i (data block j); an
 * object's answer is the block that fits every column.  That is unique
 * because no entry and no 2 x 2 minor of the coding matrix C is zero, which
 * is checked when the code's table is built (leoec_locate_wrows).
 * The limit at m = 2 is leoec_locate_dev's: two damaged blocks may be reported
 * as a third.  At k + m = 32 the bit of the last coding block (id 31) is
 * LEOEC_LOCATE_MANY's own, the limit leoec_locate_ws_dev documents: that word
 * says either, and leoec_heal_dev reads it as block 31.
 * For (c) the call allocates nothing, uploads nothing and never synchronises:
 * per chunk the class's encode into the workspace, a memset and two launches
 * on `stream`, so it can be captured into a graph, after the first call: the
 * first call of a code builds its ratio table on the host (kept for the
 * process's life, under 1 KB) and the first call on a device loads this
 * call's code object (1-2 ms); the leoec_gf_init warm-up covers neither. */
int leoec_locate_gfw_dev(int coding, int k, int m, int w, const uint8_t *objs, uint64_t obj_stride,
                         uint64_t size, uint64_t nobj, const uint8_t *parity, uint64_t parity_stride,
                         uint32_t *lost, void *workspace, uint64_t workspace_bytes, void *stream);

/* Workspace bytes leoec_scrub_dev needs for nobj objects:
 * 16 + round_up(4 * nobj, 16), a header and one index word per object;
 * LEOEC_E_BAD_SIZE when that overflows; bytes == NULL: LEOEC_E_ARG.
 * Configurations leoec_scrub_dev does not serve, and invalid ones, get its
 * statuses.  Needs no device. */
int leoec_scrub_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                              uint64_t *bytes);

/* Scrub a stored batch in one call: find the inconsistent objects, name the
 * damaged block of each, rebuild it in place and count what was found, all on
 * the device.  The contract is the composition leoec_locate_dev then
 * leoec_heal_dev(lost = report): after the call
 *   report[o]  is leoec_locate_dev's word for object o of the batch as it was
 *              before the call: 0, one bit b < k + m, or LEOEC_LOCATE_MANY;
 *   objs and parity hold the bytes leoec_heal_dev(..., lost = report, ...)
 *              leaves: every object whose word names one block has that block
 *              rebuilt in place from its first k intact ids ascending, data
 *              blocks clipped to `size`, bytes past `size` read as zero and
 *              never touched; a clean object and a LEOEC_LOCATE_MANY object
 *              are not written at all;
 *   totals[0]  is the number of objects named and rebuilt, totals[1] the number
 *              of LEOEC_LOCATE_MANY objects; both words are overwritten, so 8
 *              bytes tell whether the batch was clean.
 * Layout, alignment and stride rules are those of leoec_verify_dev and
 * leoec_heal_dev.  report: device, 4-byte aligned, nobj words, every one
 * overwritten.  totals: device, 4-byte aligned, 2 words.  workspace: device,
 * 16-byte aligned, at least leoec_scrub_dev_workspace's bytes; its contents
 * after the call are unspecified.  report, totals or workspace NULL or
 * misaligned, report or totals inside the workspace, or workspace_bytes below
 * the query's: LEOEC_E_ARG.
 * Served: what leoec_locate_dev serves, vandrs w = 8 and isars with k <= 16
 * and 2 <= m <= 4.  Everything else (cauchyrs and liberation: leoec_scrub_ws_dev;
 * vandrs w = 16 / 32, k > 16, m > 4: leoec_scrub_gfw_dev; m = 1) is
 * LEOEC_E_UNSUPPORTED, returned before the device is opened; invalid
 * parameters keep their leoec_check_params status; nobj == 0 is LEOEC_OK with
 * nothing written.  The checks come in leoec_locate_dev's order: layout and
 * parameters, served, empty batch, pointers and strides, then the device.
 * The limit at m = 2 is leoec_locate_dev's: with m >= 3 two damaged blocks are
 * never taken for one, with m = 2 they may be reported as a third block, which
 * is then "healed": the stripe is left consistent but wrong.
 * What runs: per chunk of objects leoec_locate_dev's memset and launch, one
 * launch that writes the final words and lists the objects that name a block,
 * and one launch of fixed size that rebuilds the listed objects' blocks, so
 * the repair costs by the number of damaged objects, not by the batch.
 * The call allocates nothing, uploads nothing and never synchronises, so it
 * can be captured into a graph, after the first call: the first call of a
 * code on a device builds and uploads leoec_heal_dev's pattern table (up to
 * 8 MB, a blocking copy) and loads the code objects (1-2 ms each); the
 * leoec_gf_init warm-up does not cover them.  The table cache holds 16 tables
 * per process; past that the call runs leoec_locate_dev then leoec_heal_dev's
 * other path, which brings the masks back to the host (one stream
 * synchronisation), rebuilds runs of consecutive objects with the same mask
 * and fills the workspace's index words from the host. */
int leoec_scrub_dev(int coding, int k, int m, int w, uint8_t *objs, uint64_t obj_stride,
                    uint64_t size, uint64_t nobj, uint8_t *parity, uint64_t parity_stride,
                    uint32_t *report, uint32_t *totals, void *workspace, uint64_t workspace_bytes,
                    void *stream);

/* Workspace bytes leoec_scrub_ws_dev wants for this batch: leoec_scrub_dev's
 * for everything that call serves; for cauchyrs and liberation
 * 16 + round_up(4 * nobj, 16) + nobj * m * block_size (one pass);
 * LEOEC_E_BAD_SIZE when that overflows; bytes == NULL: LEOEC_E_ARG.
 * Configurations leoec_scrub_ws_dev does not serve, and invalid ones, get its
 * statuses.  Needs no device. */
int leoec_scrub_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                 uint64_t *bytes);

/* leoec_scrub_dev with an encode region in its workspace, which adds the
 * bitmatrix classes, in the relation leoec_locate_ws_dev has to
 * leoec_locate_dev.  The contract is the composition leoec_locate_ws_dev then
 * leoec_heal_dev(lost = report), byte for byte: after the call
 *   report[o]  is leoec_locate_ws_dev's word for object o of the batch as it
 *              was before the call: 0, one bit b < k + m, or LEOEC_LOCATE_MANY;
 *   objs and parity hold the bytes leoec_heal_dev(..., lost = report, ...)
 *              leaves: every object whose word names one block has that block
 *              rebuilt in place from its first k intact ids ascending, data
 *              blocks clipped to `size`, bytes past `size` read as zero and
 *              never touched; a clean object and a LEOEC_LOCATE_MANY object
 *              are not written at all;
 *   totals[0]  is the number of objects named and rebuilt, totals[1] the number
 *              of LEOEC_LOCATE_MANY objects; both words are overwritten.
 * Layout, alignment and stride rules are leoec_scrub_dev's.
 * Served:
 *   (a) everything leoec_scrub_dev serves: the call and the query are
 *       forwarded to it, with the same workspace size, statuses and bytes;
 *   (b) cauchyrs and liberation with m >= 2, k + m <= 31 and
 *       (m-1) * k * w <= 768: leoec_locate_ws_dev's class (b) less k + m = 32,
 *       where the bit of id 31 is LEOEC_LOCATE_MANY's own word, so an object
 *       that names block 31 and one that names none could not be told apart
 *       and the totals could not be counted.
 * Everything else (vandrs w = 16 / 32 and w = 8 with k > 16 or m > 4, which
 * leoec_scrub_gfw_dev serves; m = 1, bitmatrix k + m >= 32, a table above 768
 * words such as cauchyrs(10,4,32)) is LEOEC_E_UNSUPPORTED, returned before the device is
 * opened; invalid parameters keep their leoec_check_params status; nobj == 0
 * is LEOEC_OK with nothing written.  The checks come in leoec_scrub_dev's
 * order: layout and parameters, served, empty batch, pointers and strides,
 * then the device.
 * workspace for (b): device, 16-byte aligned: a 16-byte header, then
 * round_up(4 * nobj, 16) bytes of index words, then the encode region.  The
 * query's size holds every object's m coding blocks (one pass); the call takes
 * anything down to 16 + round_up(4 * nobj, 16) + m * block_size and then works
 * in chunks of objects on the same stream, with the same results.
 * workspace_bytes below that minimum, report, totals or workspace NULL or
 * misaligned (4, 4 and 16 bytes), or report or totals inside the workspace:
 * LEOEC_E_ARG.  The workspace's contents after the call are unspecified.
 * What runs for (b), per chunk, on `stream`: the class's encode into the
 * workspace, a memset, leoec_locate_ws_dev's launch, one launch that writes
 * the final words, lists the objects that name a block and adds to the totals,
 * and one launch of fixed size that rebuilds the listed objects' blocks packet
 * by packet from the code's block table (leoec_scrub_bitrows).  Nothing is
 * allocated, uploaded or waited for, so the call can be captured into a
 * graph, after the first call: the first call of a code on a device builds
 * that table on the host (k + m records, under 100 KB), uploads it with a
 * blocking copy and loads the code objects (1-2 ms each); the leoec_gf_init
 * warm-up does not cover them.  The table cache holds 16 tables per process
 * and is its own, beside leoec_heal_dev's; past that the call runs
 * leoec_locate_ws_dev then leoec_heal_dev's other path, which brings the masks
 * back to the host (one stream synchronisation), rebuilds runs of consecutive
 * objects with the same mask and fills the workspace's index words from the
 * host.
 * The limit at m = 2 is leoec_locate_ws_dev's and holds for every liberation
 * call: two damaged blocks may be reported as a third, which is then
 * "healed". */
int leoec_scrub_ws_dev(int coding, int k, int m, int w, uint8_t *objs, uint64_t obj_stride,
                       uint64_t size, uint64_t nobj, uint8_t *parity, uint64_t parity_stride,
                       uint32_t *report, uint32_t *totals, void *workspace,
                       uint64_t workspace_bytes, void *stream);

/* Workspace bytes leoec_scrub_gfw_dev wants for this batch: for everything
 * leoec_scrub_ws_dev serves, that call's query (same value, same statuses);
 * for class (c) below 16 + round_up(4 * nobj, 16) + nobj * m * block_size
 * (one pass); LEOEC_E_BAD_SIZE when that overflows; bytes == NULL:
 * LEOEC_E_ARG, checked after the served checks.  Configurations
 * leoec_scrub_gfw_dev does not serve, and invalid ones, get its statuses.
 * Needs no device. */
int leoec_scrub_gfw_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                  uint64_t *bytes);

/* leoec_scrub_ws_dev plus the GF(2^w) word classes, in the relation
 * leoec_locate_gfw_dev has to leoec_locate_ws_dev.  The contract is the
 * composition leoec_locate_gfw_dev then leoec_heal_dev(lost = report), byte
 * for byte: after the call
 *   report[o]  is leoec_locate_gfw_dev's word for object o of the batch as it
 *              was before the call: 0, one bit b < k + m, or LEOEC_LOCATE_MANY;
 *   objs and parity hold the bytes leoec_heal_dev(..., lost = report, ...)
 *              leaves: every object whose word names one block has that block
 *              rebuilt in place from its first k intact ids ascending, data
 *              blocks clipped to `size`, bytes past `size` read as zero and
 *              never touched; a clean object and a LEOEC_LOCATE_MANY object
 *              are not written at all;
 *   totals[0]  is the number of objects named and rebuilt, totals[1] the number
 *              of LEOEC_LOCATE_MANY objects; both words are overwritten.
 * Layout, alignment and stride rules are leoec_scrub_ws_dev's.
 * Served:
 *   (a) everything leoec_scrub_ws_dev serves (its classes (a) and (b)): the
 *       call and the query are forwarded to it, with the same workspace size,
 *       statuses and bytes; the bitmatrix configurations it refuses stay
 *       refused;
 *   (c) vandrs w = 16 / 32, and vandrs / isars w = 8 with k > 16 or m > 4, all
 *       with m >= 2 and k + m <= 31: leoec_locate_gfw_dev's class (c) less
 *       k + m = 32, where the bit of id 31 is LEOEC_LOCATE_MANY's own word,
 *       the reason leoec_scrub_ws_dev gives.
 * Everything else (m = 1, k + m >= 32, the bitmatrix configurations
 * leoec_scrub_ws_dev refuses) is LEOEC_E_UNSUPPORTED, returned before the
 * device is opened; invalid parameters keep their leoec_check_params status;
 * nobj == 0 is LEOEC_OK with nothing written.  The checks come in
 * leoec_scrub_ws_dev's order: layout and parameters, served, empty batch,
 * pointers and strides, workspace, then the device.
 * workspace for (c): leoec_scrub_ws_dev's layout: device, 16-byte aligned: a
 * 16-byte header, then round_up(4 * nobj, 16) bytes of index words, then the
 * encode region.  The query's size holds every object's m coding blocks (one
 * pass); the call takes anything down to 16 + round_up(4 * nobj, 16) +
 * m * block_size and then works in chunks of objects on the same stream, with
 * the same results.  workspace_bytes below that minimum, report, totals or
 * workspace NULL or misaligned (4, 4 and 16 bytes), or report or totals inside
 * the workspace: LEOEC_E_ARG.  The workspace's contents after the call are
 * unspecified.
 * What runs for (c), per chunk, on `stream`: the class's encode into the
 * workspace, a memset, leoec_locate_gfw_dev's launch, one launch that writes
 * the final words, lists the objects that name a block and adds to the totals,
 * and one launch of fixed size that rebuilds the listed objects' blocks on
 * w-bit words from the code's block table (leoec_scrub_wrows).  Nothing is
 * allocated, uploaded or waited for, so the call can be captured into a
 * graph, after the first call: the first call of a code on a device builds
 * that table on the host (k + m records, under 5 KB), uploads it with a
 * blocking copy and loads the code objects (1-2 ms each); the leoec_gf_init
 * warm-up does not cover them.  The table cache holds 16 tables per process
 * and is its own, beside leoec_heal_dev's and leoec_scrub_ws_dev's; past that
 * the call runs leoec_locate_gfw_dev then leoec_heal_dev's other path, which
 * brings the masks back to the host (one stream synchronisation), rebuilds
 * runs of consecutive objects with the same mask and fills the workspace's
 * index words from the host.
 * The limit at m = 2 is leoec_locate_dev's: with m >= 3 two damaged blocks are
 * never taken for one, with m = 2 they may be reported as a third block, which
 * is then "healed": the stripe is left consistent but wrong. */
int leoec_scrub_gfw_dev(int coding, int k, int m, int w, uint8_t *objs, uint64_t obj_stride,
                        uint64_t size, uint64_t nobj, uint8_t *parity, uint64_t parity_stride,
                        uint32_t *report, uint32_t *totals, void *workspace,
                        uint64_t workspace_bytes, void *stream);

/* ---- introspection ------------------------------------------------------ */

/* The map leoec_scrub_gfw_dev rebuilds one lost block of an object of its
 * class (c) with; needs no device.  surv[0..k): the first k ids ascending
 * without `block`, leoec_decode_dev's survivors.  coef[0..k) (cap >= k words):
 * the GF(2^w) coefficients that give `block` from the blocks surv[0..k) in
 * that order, word by word: a record of the table the device holds, equal to
 * leoec_heal_rows' surv and coef for the mask 1 << block.  A block outside
 * 0..k+m-1: LEOEC_E_BAD_ID; surv or coef NULL or cap too small: LEOEC_E_ARG.
 * Serves class (c) of leoec_scrub_gfw_dev only and gives its statuses
 * otherwise; class (a) is LEOEC_E_UNSUPPORTED (those maps are leoec_heal_rows
 * and leoec_scrub_bitrows). */
int leoec_scrub_wrows(int coding, int k, int m, int w, int block, int *surv, uint32_t *coef,
                      int cap);

/* The map leoec_scrub_ws_dev rebuilds one lost block of a cauchyrs or
 * liberation object with; needs no device.  surv[0..k): the first k ids
 * ascending without `block`, leoec_decode_dev's survivors.  rows
 * (cap >= w * ceil(k*w / 32) words): row r is ceil(k*w / 32) words; bit
 * i*w + c of the row (word (i*w + c) / 32, bit (i*w + c) % 32) is set iff
 * packet c of block surv[i] feeds packet r of `block`.  A block outside
 * 0..k+m-1: LEOEC_E_BAD_ID; surv or rows NULL or cap too small: LEOEC_E_ARG.
 * Serves class (b) of leoec_scrub_ws_dev only and gives its statuses
 * otherwise; vandrs and isars are LEOEC_E_UNSUPPORTED (their map is
 * leoec_heal_rows). */
int leoec_scrub_bitrows(int coding, int k, int m, int w, int block, int *surv, uint32_t *rows,
                        int cap);

/* leoec_scrub_bitrows for a mask: the map leoec_heal_ws_dev rebuilds the r-th
 * lost id (ascending, r from 0) of lost_mask of a cauchyrs or liberation
 * object with, read from the table the device holds; needs no device.
 * surv[0..k): the first k intact ids ascending; rows: leoec_scrub_bitrows'
 * format (cap >= w * ceil(k*w / 32) words).  For a mask of one bit surv and
 * rows are leoec_scrub_bitrows' for that block.  A bit at or above k + m:
 * LEOEC_E_BAD_ID; more than m bits: LEOEC_E_NOT_ENOUGH_BLOCKS (leoec_heal_rows'
 * statuses); r outside the mask's bit count, surv or rows NULL or cap too
 * small: LEOEC_E_ARG.  Serves the cauchyrs and liberation codes
 * leoec_heal_ws_dev serves and gives its statuses otherwise; vandrs and isars
 * are LEOEC_E_UNSUPPORTED (their map is leoec_heal_rows). */
int leoec_heal_bitrows(int coding, int k, int m, int w, uint32_t lost_mask, int r, int *surv,
                       uint32_t *rows, int cap);

/* leoec_scrub_wrows for a mask: the map leoec_heal_ws_dev rebuilds the r-th
 * lost id (ascending, r from 0) of lost_mask with for a vandrs or isars code
 * outside leoec_heal_dev's fused family (w = 16 / 32, w = 8 with k > 16 or
 * m > 4), read from the table the device holds; needs no device.
 * surv[0..k): the first k intact ids ascending; coef[0..k) (cap >= k words):
 * the GF(2^w) coefficients that give the lost block from those survivors,
 * equal to leoec_heal_rows' surv and row r of its coef for the same mask.
 * Statuses as leoec_heal_bitrows'; cauchyrs, liberation and the fused family
 * are LEOEC_E_UNSUPPORTED (their maps are leoec_heal_bitrows and
 * leoec_heal_rows). */
int leoec_heal_wrows(int coding, int k, int m, int w, uint32_t lost_mask, int r, int *surv,
                     uint32_t *coef, int cap);

/* The GF(2) ratios leoec_locate_ws_dev tests the syndromes of cauchyrs and
 * liberation with; needs no device.  rows (cap >= (m-1) * k * w words): word
 * ((i-1) * k + j) * w + r is row r of T[i][j] = B[i][j] B[0][j]^-1, i = 1..m-1;
 * bit c (bit 0 = packet 0) is set iff syndrome packet c of coding block 0
 * feeds the prediction of packet r of coding block i.  rows == NULL or cap too
 * small: LEOEC_E_ARG.  Serves class (b) of leoec_locate_ws_dev only and gives
 * its statuses otherwise; vandrs and isars are LEOEC_E_UNSUPPORTED (their
 * table is leoec_locate_rows).  While building T the two properties the
 * answer's uniqueness rests on are checked (every block and every 2w x 2w
 * minor invertible): LEOEC_E_UNSUPPORTED if either fails. */
int leoec_locate_bitrows(int coding, int k, int m, int w, uint32_t *rows, int cap);

/* The ratios leoec_locate_dev tests the syndromes with; needs no device.
 * ratio (cap >= (m-1) * k words): row i-1 holds T[i][0..k) = C[i][j] / C[0][j]
 * in GF(2^8), i = 1..m-1, C being leoec_coding_matrix's.  ratio == NULL or
 * cap too small: LEOEC_E_ARG.  Configurations leoec_locate_dev does not serve
 * get its statuses.  While building T the two properties the answer's
 * uniqueness rests on are checked (no zero entry, no singular 2 x 2 minor of
 * C): LEOEC_E_UNSUPPORTED if either fails. */
int leoec_locate_rows(int coding, int k, int m, int w, uint32_t *ratio, int cap);

/* The ratios leoec_locate_gfw_dev tests the syndromes of its class (c) with;
 * needs no device.  ratio (cap >= (m-1) * k words): word (i-1) * k + j is
 * T[i][j] = C[i][j] / C[0][j] in GF(2^w), i = 1..m-1, C being
 * leoec_coding_matrix's.  ratio == NULL or cap too small: LEOEC_E_ARG.  Serves
 * class (c) of leoec_locate_gfw_dev only and gives its statuses otherwise;
 * class (a) is LEOEC_E_UNSUPPORTED (those tables are leoec_locate_rows and
 * leoec_locate_bitrows).  While building T the two properties the answer's
 * uniqueness rests on are checked (no zero entry, no singular 2 x 2 minor of
 * C): LEOEC_E_UNSUPPORTED if either fails. */
int leoec_locate_wrows(int coding, int k, int m, int w, uint32_t *ratio, int cap);

/* The map leoec_heal_dev uses for one mask of lost ids; needs no device.
 * surv[0..k): the survivor ids; want[0..*nwant): the lost ids ascending;
 * coef (may be NULL; cap >= *nwant * k words): row r holds the GF(2^w)
 * coefficients that give block want[r] from the survivor blocks in surv's
 * order (liberation has no such matrix: LEOEC_E_UNSUPPORTED when coef is
 * given).  *index (may be NULL): the mask's record in the device table of the
 * one-launch configurations (its combinatorial rank: masks of fewer bits
 * first, then sum over the set bits b_1 < b_2 < ... of C(b_i, i)); -1 for
 * every other configuration and for mask 0.
 * A bit at or above k+m: LEOEC_E_BAD_ID; more than m bits:
 * LEOEC_E_NOT_ENOUGH_BLOCKS; k + m > 32: LEOEC_E_UNSUPPORTED. */
int leoec_heal_rows(int coding, int k, int m, int w, uint32_t lost_mask, int *surv, int *want,
                    int *nwant, uint32_t *coef, int cap, int *index);

/* Coding matrix the engine uses: m*k words (GF classes) or a (m*w) x (k*w)
 * 0/1 bitmatrix as bytes (cauchyrs, liberation).  *n_out = entries written. */
int leoec_coding_matrix(int coding, int k, int m, int w, uint32_t *out, int cap, int *n_out);

/* Device ordinal the calling thread's device-resident calls (*_dev) use,
 * or a negative status. */
int leoec_device(void);

/* Host-memory calls (leoec_encode / _decode / _repair) run on the calling
 * thread's current HIP device by default (each device has its own batching
 * queue, its dispatcher lane).  Returns the number of lanes (one per gfx950
 * device visible to the process) and writes the device ordinal of lane i to
 * devices[i] for i < cap (devices may be NULL), or a negative status.
 * (No reference counterpart: the reference is CPU-only.) */
int leoec_host_lanes(int *devices, int cap);

/* Opt in to spreading host-memory calls over several devices: with n > 0,
 * each later call goes to the device of devices[0..n-1] whose lane has the
 * fewest calls in progress (its own queue and PCIe link), and the caller's
 * current device is left as it was; n == 0 restores the default (the
 * caller's current device).  Every ordinal must be a gfx950 device visible
 * to the process (else LEOEC_E_NO_DEVICE, and the setting is unchanged).
 * Returns the number of devices in the set.  Only the devices of the set get
 * queues and pinned arenas (5 x 32 MiB pinned + 5 x 32 MiB device each), and
 * each of them is warmed before this returns, as gf_init warms the caller's
 * device (its hardware queues, code objects, batching queue and pools, one
 * thread per device: ~0.3 s once), so no device's first call pays that.
 * (No reference counterpart: the reference is CPU-only.) */
int leoec_host_spread(const int *devices, int n);

/* Library version string. */
const char *leoec_version(void);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* LEOEC_H */
