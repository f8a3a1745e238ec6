"""GPU: every upload path puts every row of every array into its slot.

Everything the library computes starts from upload_common (sba_shim.cpp) or batch_transfer (sba_batch.cpp): the only
device paths with chunking, double buffering, events and a pool of host threads.  The other files see them through
reductions at the sizes where those mechanisms run, and a reduction cannot see rows exchanged alike in left, right and
depths.  Here the inputs name their own rows (tests/upload_patterns.py): one residual call at rot = tran = 0 and uniform
depths 1 returns e = x2 - x1, which says for every slot which source row of x1 and of x2 the planes hold, and a joint
solve that may not iterate hands the depth planes back untouched (tests/test_gpu_resection.py, test_gpu_batch_joint.py).
Every row of every case is compared: against the long-double restatement under the 1e-12 bound of
tests/test_gpu_residuals.py, and bit for bit (the codes make x2 - x1 exact in float64, and no operation of the residual
kernel rounds at R = I, t = 0, d = 1).  A failure names the array, the row, its chunk and the offset in the chunk."""
import numpy as np
import pytest

import upload_patterns as up
from spherical_bundle_adjuster_amd import api, synthetic

pytestmark = pytest.mark.gpu

PIPELINED_MIN = 1 << 21          # sba_shim.cpp:687 kPipelinedUploadMin: matches from which the pipelined path runs
CHUNK = 699050                   # sba_shim.cpp:688 kUploadChunk: rows per pipelined chunk (16 MiB of xyz); CHUNK % 4 == 2
SINGLE_CHUNK = 4 << 20           # sba_shim.cpp:717: rows per chunk of the single-buffer path
BATCH_CHUNK = 699050             # sba_batch.cpp:357 kBatchUploadChunk
POOL_MIN_BYTES = 8 << 20         # sba_batch.cpp:374: total * 24 below this -> one copy thread
POOL_MIN_ROWS = -(-POOL_MIN_BYTES // 24)     # 349 526: the first batch size that gets the copy pool
STORES = (api.STORE_F64, api.STORE_F32)
IDS = ("f64", "f32")
ZERO = np.zeros(3)
TRAN = np.array([0.0, 0.0, 1.0])             # the joint solve's gauge pins |t|: any unit translation serves the read-back
NO_STEP = dict(max_num_iterations=0, tran_param=api.TRAN_SPHERE)

assert CHUNK % 4 == 2 and PIPELINED_MIN == 3 * CHUNK + 2 and POOL_MIN_ROWS == 349526


@pytest.fixture(scope="module")
def source():
    """The rows of the largest case, built once; every case uploads a prefix (or a slice: its rows then start at row0)."""
    return up.patterns(SINGLE_CHUNK + 3)


def _read(p, with_depths=True):
    """(e, d12) of a problem: the residuals at rot = tran = 0, d = 1 and the depth planes as they are."""
    e = p.residuals(ZERO, ZERO, 1.0, 1.0, huber_delta=0.0, depth_mode=api.DEPTH_UNIFORM, fields=("e",)).e
    d = None
    if with_depths:
        _, _, d, s = p.solve_joint(ZERO, TRAN, options=api.default_lm_options(**NO_STEP))
        assert s.num_iterations == 0 and s.num_successful_steps == 0
    return e, d


def _upload_and_check(p, source, n, store, chunk, what, depths="with", row0=0):
    left, right, d12 = (a[row0:row0 + n] for a in source)
    if depths == "with":
        p.upload(left, right, d12, store=store)
    else:
        p.upload(left, right, None, store=store)
        if depths == "later":
            # before the depths arrive the rows are already in place
            up.check_rows(_read(p, False)[0], None, n, chunk, row0=row0, what=what + " before set_depths")
            p.set_depths(d12)
    assert p.size == n
    e, d = _read(p, depths != "without")
    up.check_rows(e, d, n, chunk, row0=row0, what=what)
    return e, d


# ---- single problem, pipelined path -----------------------------------------------------------------------------------------
PIPELINED_SIZES = [PIPELINED_MIN - 1,    # the last size of the single-buffer path
                   PIPELINED_MIN,        # three full chunks and a two-row chunk
                   4 * CHUNK - 1, 4 * CHUNK,      # an exact multiple: no ragged chunk
                   4 * CHUNK + 1]        # ends in a one-row chunk


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("n", PIPELINED_SIZES)
def test_pipelined_upload_rows(source, n, store):
    with api.Problem(0) as p:
        _upload_and_check(p, source, n, store, CHUNK, f"n={n} store={store}")


def test_pipelined_upload_without_depths(source):
    """Two jobs instead of three: the right array's chunks start at pinned buffer 0 again (k = 4), not at buffer 1."""
    with api.Problem(0) as p:
        _upload_and_check(p, source, PIPELINED_MIN, api.STORE_F32, CHUNK, "no d12", depths="without")


def test_pipelined_upload_depths_later(source):
    with api.Problem(0) as p:
        _upload_and_check(p, source, PIPELINED_MIN, api.STORE_F64, CHUNK, "d12 by set_depths", depths="later", row0=5)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_upload_thread_counts(monkeypatch, source, store):
    """1, 5 and 6 copy threads: shares of CHUNK * 24 bytes that do not divide, and at the one-row last chunk (24 and 16
    bytes) every thread but the first gets an empty share.  All three give the same bytes."""
    n = 4 * CHUNK + 1
    got = []
    for threads in (1, 5, 6):
        monkeypatch.setenv("SBA_UPLOAD_THREADS", str(threads))
        with api.Problem(0) as p:
            got.append(_upload_and_check(p, source, n, store, CHUNK, f"{threads} threads store={store}"))
    for e, d in got[1:]:
        assert e.tobytes() == got[0][0].tobytes() and d.tobytes() == got[0][1].tobytes()


# ---- single-buffer path past one chunk -----------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_single_buffer_second_chunk(monkeypatch, source, store):
    """SBA_UPLOAD_PIPELINE=0 and n > 4 Mi: the only way into the second trip of the single-buffer loops, first != 0 in
    launch_aos_to_planes / launch_d12_to_planes (a three-row chunk: inside one f32 vector)."""
    monkeypatch.setenv("SBA_UPLOAD_PIPELINE", "0")
    with api.Problem(0) as p:
        _upload_and_check(p, source, SINGLE_CHUNK + 3, store, SINGLE_CHUNK, f"single buffer store={store}")


# ---- re-upload into a handle that held a larger problem ---------------------------------------------------------------------
@pytest.fixture
def pinned_grid(monkeypatch):
    """Same blocks per CU for every sweep variant (read at handle creation): two handles then reduce in the same order and
    their packs compare bit for bit (tests/test_gpu_residuals.py)."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


def _bits(*arrays):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)


def _state(p, c):
    """Everything compared between a re-used and a fresh handle: rows, depths, pack, resection and joint equations."""
    r = p.residuals(c.rot_init, c.tran_init, huber_delta=1.0, depth_mode=api.DEPTH_PER_MATCH)
    pack = p.eval_pack(api.MODE_RT, c.rot_init, c.tran_init, huber_delta=1.0, depth_mode=api.DEPTH_PER_MATCH)
    rs = p.eval_resection(c.rot_init, c.tran_init)
    j = p.eval_joint(c.rot_init, c.tran_init)
    _, _, d, _ = p.solve_joint(c.rot_init, c.tran_init, options=api.default_lm_options(**NO_STEP))
    assert np.isfinite(pack).all() and np.isfinite(rs.H).all() and np.isfinite(j.S).all() and pack[22] > 0
    return _bits(r.e, r.sq_norm, r.inlier, [r.n_inlier], pack, rs.H, rs.g, [rs.cost, rs.sum_w, rs.n_outlier, rs.n_behind],
                 j.S, j.gs, j.V, j.gc, [j.cost, j.sum_w, j.n_outlier, j.gd_max], d)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_reupload_smaller_equals_fresh(pinned_grid, source, store):
    """A large pipelined problem, then smaller ragged ones (n % 4 = 1, 2, 3; the first still pipelined) into the same
    handle: the planes, pinned buffers and events are re-used, and nothing of the larger problem may show."""
    big = 4 * CHUNK + 1
    smaller = (PIPELINED_MIN + 1, 1_000_002, 65_539)
    assert [n % 4 for n in smaller] == [1, 2, 3]
    with api.Problem(0) as p:
        _upload_and_check(p, source, big, store, CHUNK, "the large problem")
        for n in smaller:
            # its own rows, from further down the source: a row the large problem left behind would name itself
            chunk = CHUNK if n >= PIPELINED_MIN else SINGLE_CHUNK
            _upload_and_check(p, source, n, store, chunk, f"re-upload n={n} store={store}", row0=big - n - 7)
        for n in smaller[1:]:
            c = synthetic.full_rt(n, seed=synthetic.BASE_SEED + 900 + n % 4, outlier_fraction=0.1)
            p.upload(source[0][:big], source[1][:big], source[2][:big], store=store)
            p.upload(c.x1, c.x2, c.d12, store=store)
            with api.Problem(0) as q:
                q.upload(c.x1, c.x2, c.d12, store=store)
                assert _state(p, c) == _state(q, c), n


# ---- upload_device ----------------------------------------------------------------------------------------------------------
def test_upload_device_rows(source):
    import torch
    n = PIPELINED_MIN + 1
    dev = [torch.from_numpy(a[3:3 + n]).to("cuda:0") for a in source]
    torch.cuda.synchronize()
    for store in STORES:
        with api.Problem(0) as p:
            p.upload_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n, store=store)
            e, d = _read(p)
            up.check_rows(e, d, n, CHUNK, row0=3, what=f"upload_device store={store}")


# ---- batches ------------------------------------------------------------------------------------------------------------------
def _multi_chunk_offsets():
    """Pair boundaries (relative to offsets[0]) around the chunk boundaries of a batch a little above 3 chunks."""
    C = BATCH_CHUNK
    b = [0, 2049, 2054, 2054, 2054,                 # 2049 and 5 rows, then two consecutive empty pairs
         C - 4, C - 1,                              # ... a pair of 3 rows up to C - 1
         C, C + 1, C + 3,                           # boundaries at C - 1, C and C + 1: pairs of 1, 1 and 2 rows
         2 * C - 2049, 2 * C, 2 * C,                # 2049 rows up to the boundary, and an empty pair ON it
         2 * C + 5,                                 # 5 rows after it
         3 * C + 12,                                # a pair of C + 7 rows: longer than a chunk, chunk 3 starts inside it
         3 * C + 15, 3 * C + 17, 3 * C + 34]        # 3 and 2 rows, and a last pair of 17 rows: a last chunk of 34 rows
    sizes = np.diff(b)
    assert (sizes >= 0).all() and {0, 1, 2, 3, 5, 2049} <= set(sizes.tolist()) and sizes.max() > C
    assert {C - 1, C, C + 1} <= set(b) and b.count(2 * C) == 2 and b.count(2054) == 3 and 0 < b[-1] % C < 64
    return np.array(b, dtype=np.uint64)


def _read_batch(b, with_depths=True):
    B = b.num_pairs
    z = np.zeros((B, 3))
    e = b.residuals(z, z, np.ones(B), np.ones(B), huber_delta=0.0, depth_mode=api.DEPTH_UNIFORM, fields=("e",)).e
    d = None
    if with_depths:
        # check=False: what an empty or a tiny pair's solver makes of these inputs is not the subject; the planes come back
        d = b.solve_joint(z, np.tile(TRAN, (B, 1)), options=api.default_lm_options(**NO_STEP), check=False)[2]
    return e, d


def _batch_upload_and_check(b, source, off, store, what, with_depths=True, shift=0):
    """Upload rows shift .. shift + off[-1] of the source as the batch's arrays (pair g at off[g]); slot j must then hold
    source row shift + off[0] + j."""
    base, end = int(off[0]), int(off[-1])
    left, right, d12 = (a[shift:shift + end] for a in source)
    b.upload(left, right, off, d12 if with_depths else None, store=store)
    e, d = _read_batch(b, with_depths)
    if d is not None:
        assert d.shape == (end, 2) and not d[:base].any()         # indexed like the uploaded arrays
        d = d[base:]
    up.check_rows(e, d, end - base, BATCH_CHUNK, row0=shift + base, what=what)
    return e, d


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_batch_multi_chunk_rows(source, store):
    with api.Batch(0) as b:
        _batch_upload_and_check(b, source, _multi_chunk_offsets(), store, f"batch store={store}")
        # the same pairs again with other rows: the layout stays and only the data moves (sba_batch_upload's short cut)
        _batch_upload_and_check(b, source, _multi_chunk_offsets(), store, f"same pairs again store={store}", shift=11)


def test_batch_multi_chunk_rows_from_an_offset(source):
    """offsets[0] != 0: the arrays' first rows belong to no pair, and every boundary above is relative to offsets[0]."""
    with api.Batch(0) as b:
        _batch_upload_and_check(b, source, _multi_chunk_offsets() + np.uint64(7), api.STORE_F32, "batch from row 7")


def _small_offsets(total):
    b = [0, 1, 3, 2052, 2052, total // 2 + 1, total - 5, total]
    return np.array(b, dtype=np.uint64)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_batch_set_depths_moves_only_the_depths(source, store):
    """The `which` mask of batch_transfer: set_depths sends the d12 job alone.  The batch API takes new depths only where
    depths were uploaded (without them it refuses, and the refusal leaves the rows alone), so: upload with one set of
    depths, replace them with another, and the x rows must not move by a bit."""
    off = _multi_chunk_offsets()
    total = int(off[-1])
    later = up.depth_codes(np.arange(total, 2 * total))            # the depths of other rows: nothing of the first set may stay
    with api.Batch(0) as b:
        e0, _ = _batch_upload_and_check(b, source, off, store, "before set_depths")
        b.set_depths(later)
        e1, d1 = _read_batch(b)
        assert e1.tobytes() == e0.tobytes()
        up.check_rows(e1, None, total, BATCH_CHUNK, what="x rows after set_depths")
        for col in (0, 1):
            rows, kind = up.decode_depth(d1[:, col])
            bad = np.flatnonzero((rows != np.arange(total, 2 * total)) | (kind != col + 1))
            assert bad.size == 0, (f"d{col + 1} after set_depths: first bad row {bad[0]} = chunk {bad[0] // BATCH_CHUNK} + "
                                   f"{bad[0] % BATCH_CHUNK} holds {d1[bad[0], col]!r}; {bad.size} bad rows")
    with api.Batch(0) as b:
        e0, _ = _batch_upload_and_check(b, source, off, store, "without depths", with_depths=False)
        with pytest.raises(api.SbaError) as ei:
            b.set_depths(later)
        assert ei.value.code == api.cabi.SBA_ERR_INVALID_ARG
        assert _read_batch(b, False)[0].tobytes() == e0.tobytes()


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("total", [POOL_MIN_ROWS - 1, POOL_MIN_ROWS], ids=["one_thread", "copy_pool"])
def test_batch_single_chunk_either_side_of_the_pool_rule(source, total, store):
    """One chunk of total * 24 bytes just below 8 MiB (one copy thread) and just above (the pool: six shares of a byte
    count that does not divide)."""
    assert (total * 24 < POOL_MIN_BYTES) == (total == POOL_MIN_ROWS - 1) and total < BATCH_CHUNK
    with api.Batch(0) as b:
        _batch_upload_and_check(b, source, _small_offsets(total), store, f"batch of {total} rows store={store}")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_batch_reupload_smaller_equals_fresh(source, store):
    """A smaller batch into a handle that held a larger one: a fresh layout, the pinned buffers and events re-used."""
    small = _small_offsets(POOL_MIN_ROWS + 2)
    with api.Batch(0) as b, api.Batch(0) as q:
        _batch_upload_and_check(b, source, _multi_chunk_offsets(), store, "the large batch")
        e, d = _batch_upload_and_check(b, source, small, store, "the smaller batch re-uploaded")
        ef, df = _batch_upload_and_check(q, source, small, store, "the smaller batch, fresh")
        assert e.tobytes() == ef.tobytes() and d.tobytes() == df.tobytes()
        # ... and the sweeps over them: realistic rows, so that the packs are finite and say something
        cs = [synthetic.full_rt(int(n), seed=synthetic.BASE_SEED + 950 + g, outlier_fraction=0.1) for g, n in enumerate((5, 2049, 0, 70_001))]
        off = np.concatenate([[0], np.cumsum([c.x1.shape[0] for c in cs])]).astype(np.uint64)
        x1, x2, d12 = (np.concatenate([getattr(c, k) for c in cs]) for k in ("x1", "x2", "d12"))
        rot, tran = np.stack([c.rot_init for c in cs]), np.stack([c.tran_init for c in cs])
        b.upload(x1, x2, off, d12, store=store)
        q.upload(x1, x2, off, d12, store=store)
        pb, pq = (h.eval(api.MODE_RT, rot, tran, depth_mode=api.DEPTH_PER_MATCH) for h in (b, q))
        assert np.isfinite(pb).all() and pb.tobytes() == pq.tobytes()
