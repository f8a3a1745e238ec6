"""CPU: the row-identifying upload inputs (tests/upload_patterns.py) and the sensitivity of their checker.

The codes must be unique and survive float32; the decoder must invert them; and the checker must see -- and name the
array, chunk and offset of -- every kind of misplacement the chunked upload paths could produce.  The faults are injected
into a byte-level numpy model of the pipelined upload (sba_shim.cpp: upload_common; sba_batch.cpp: batch_transfer): jobs
left, right, d12; chunks of CHUNK rows; two pinned buffers used alternately over ALL chunks of all jobs; a copy pool
whose thread t copies bytes [per * t, per * (t + 1)) with per = the share rounded up to 64 bytes; the re-layout writing
rows first .. first + m of the planes."""
import numpy as np
import pytest

import upload_patterns as up

CHUNK = 699050           # sba_shim.cpp kUploadChunk, sba_batch.cpp kBatchUploadChunk
THREADS = 6              # copy threads of both paths unless SBA_UPLOAD_THREADS
N = 3 * CHUNK + 2        # three full chunks and a two-row chunk, like the smallest pipelined problem's tail


def model_upload(left, right, d12, chunk=CHUNK, threads=THREADS, src_shift=None, first_of=None, stale=None, drop=None):
    """Planes (x1 (n, 3), x2 (n, 3), d (n, 2)) after the modelled pipelined upload.  Faults, each keyed by (job, chunk
    number within the job) with job 0 left, 1 right, 2 d12:
      src_shift {(job, c): rows}   the chunk's host source starts that many rows off
      first_of  {(job, c): c2}     the re-layout gets chunk c2's first row
      stale     {(job, c): t}      copy thread t leaves the last 64 bytes of its share as the pinned buffer held them
      drop      {(job, c)}         the chunk is never sent"""
    src_shift, first_of, stale, drop = src_shift or {}, first_of or {}, stale or {}, drop or set()
    n = left.shape[0]
    srcs = [np.ascontiguousarray(a) for a in (left, right, d12)]
    planes = [np.zeros_like(a) for a in srcs]
    pinned = [np.zeros(chunk * 24, dtype=np.uint8), np.zeros(chunk * 24, dtype=np.uint8)]
    k = 0
    for job, src in enumerate(srcs):
        width = src.shape[1]
        raw = src.view(np.uint8).reshape(-1)
        for c, first in enumerate(range(0, n, chunk)):
            m = min(chunk, n - first)
            nbytes = m * width * 8
            buf = pinned[k & 1]
            k += 1
            if (job, c) in drop:
                continue
            begin = (first + src_shift.get((job, c), 0)) * width * 8
            per = ((nbytes + threads - 1) // threads + 63) & ~63
            for t in range(threads):
                lo, hi = min(nbytes, per * t), min(nbytes, per * (t + 1))
                if stale.get((job, c)) == t:
                    hi = max(lo, hi - 64)
                buf[lo:hi] = raw[begin + lo:begin + hi]
            dst = chunk * first_of[(job, c)] if (job, c) in first_of else first
            planes[job][dst:dst + m] = buf[:nbytes].view(np.float64).reshape(m, width)
    return planes


def restate(planes):
    """What the device hands back: e = x2 - x1 in float64 (exact for the codes) and the depths as they are."""
    x1, x2, d = planes
    return x2 - x1, d


@pytest.fixture(scope="module")
def source():
    return up.patterns(N)


@pytest.fixture(scope="module")
def clean(source):
    return model_upload(*source)


def _copy(planes):
    return [a.copy() for a in planes]


def _fault(planes, **kw):
    e, d = restate(planes)
    return up.first_fault(e, d, e.shape[0], CHUNK, **kw)


# ---- the codes ---------------------------------------------------------------------------------------------------------
def test_codes_are_unique_and_survive_float32():
    i = np.arange(up.MAX_ROWS, dtype=np.int64)
    for codes in (up.left_codes, up.right_codes):
        c = codes(i)
        assert np.array_equal(c.astype(np.float32).astype(np.float64), c)
        key = np.round(c[:, 0] * (1 if c[0, 0] >= 1 else up.GRID)).astype(np.int64) - 1 \
            + ((np.round(c[:, 1] * (1 if c[0, 1] >= 1 else up.GRID)).astype(np.int64) - 1) << 12)
        assert np.array_equal(key, i)                       # x and y alone name the row
        assert c.min() > 0
    d = up.depth_codes(i)
    # no value twice, in or across the columns: both increase strictly and their ranges do not meet
    assert np.all(np.diff(d[:, 0]) > 0) and np.all(np.diff(d[:, 1]) > 0)
    assert d.min() > 0 and d[:, 0].max() <= 1.0 < d[:, 1].min() and d[:, 1].max() <= 2.0
    # left and right do not meet either: fractions up to 1 against integers from 1, and the z codes keep them apart at 1
    assert not np.any((up.left_codes(i) == 1.0).all(axis=1))


def test_decode_of_the_restatement_is_the_identity():
    for row0, n in ((0, 70_001), (up.MAX_ROWS - 70_001, 70_001), (4093 * 4091 - 5, 11)):
        left, right, d12 = up.patterns(n, row0)
        want = np.arange(row0, row0 + n)
        for x1, x2 in ((left, right), (left.astype(np.float32).astype(np.float64), right.astype(np.float32).astype(np.float64))):
            e = up.reference_e(x1, x2)
            e64 = e.astype(np.float64)
            assert np.array_equal(e64.astype(np.longdouble), e)          # exact in float64
            lrow, rrow = up.decode_e(e64)
            assert np.array_equal(lrow, want) and np.array_equal(rrow, want)
        for col in (0, 1):
            rows, kind = up.decode_depth(d12[:, col])
            assert np.array_equal(rows, want) and np.all(kind == col + 1)
        assert up.first_fault(right - left, d12, n, CHUNK, row0=row0) is None
        assert up.first_fault(right - left, None, n, CHUNK, row0=row0) is None
    with pytest.raises(ValueError):
        up.patterns(2, up.MAX_ROWS - 1)


def test_the_model_without_a_fault_is_clean(source):
    for threads in (1, 5, 6):
        assert _fault(model_upload(*source, threads=threads)) is None


# ---- every simulated fault is seen, and named ------------------------------------------------------------------------------
@pytest.mark.parametrize("job", [0, 1, 2], ids=["left", "right", "d12"])
def test_chunk_source_shifted_by_one_row(source, job):
    f = _fault(model_upload(*source, src_shift={(job, 1): -1}))
    assert (f.array, f.row, f.chunk, f.offset) == (("x1", "x2", "d1")[job], CHUNK, 1, 0), f
    assert f.n_bad == CHUNK and f.last == 2 * CHUNK - 1 and "shifted by -1" in f.hint and f"row {CHUNK - 1}" in f.found, f


@pytest.mark.parametrize("job", [0, 1, 2], ids=["left", "right", "d12"])
def test_two_chunks_swapped(source, job):
    f = _fault(model_upload(*source, first_of={(job, 1): 2, (job, 2): 1}))
    assert (f.array, f.row, f.chunk, f.offset) == (("x1", "x2", "d1")[job], CHUNK, 1, 0), f
    assert f.n_bad == 2 * CHUNK and "chunk 2" in f.hint and f"row {2 * CHUNK}" in f.found, f


@pytest.mark.parametrize("job,c,t", [(0, 2, 1), (1, 1, 5), (2, 2, 0), (0, 1, 3)])
def test_last_64_bytes_of_a_share_left_stale(source, job, c, t):
    width = 3 if job < 2 else 2
    nbytes = CHUNK * width * 8
    per = ((nbytes + THREADS - 1) // THREADS + 63) & ~63
    hi = min(nbytes, per * (t + 1))
    e, d = restate(model_upload(*source, stale={(job, c): t}))
    first = up.first_fault(e, d, N, CHUNK)
    assert first is not None and (first.chunk, first.offset) == (c, (hi - 64) // (8 * width)), first
    assert "stale" in first.hint or first.array[0] == "d", first
    # the job's own array is among the blamed ones.  The stale bytes are the other side's rows of the same slots wherever the
    # pinned buffer last carried that side (e = 0 there): which plane is off cannot be told from e, and both are named.
    own = [f for f in up.all_faults(e, d, N, CHUNK) if f.array in (("x1",), ("x2",), ("d1", "d2"))[job]]
    assert own and all((f.array[0] == "d") == (job == 2) for f in up.all_faults(e, d, N, CHUNK)), own
    f = own[0]
    assert (f.chunk, f.offset) == (c, (hi - 64) // (8 * width)), f
    assert f.n_bad <= 64 // (8 * width) + 2 and f.last < c * CHUNK + -(-hi // (8 * width)), f


@pytest.mark.parametrize("job", [0, 1, 2], ids=["left", "right", "d12"])
def test_two_row_last_chunk_dropped(source, job):
    f = _fault(model_upload(*source, drop={(job, 3)}))
    assert (f.array, f.row, f.chunk, f.offset, f.n_bad) == (("x1", "x2", "d1")[job], 3 * CHUNK, 3, 0, 2), f
    assert f.found.startswith("zero") and "never written" in f.hint, f


def test_left_and_right_exchanged(source, clean):
    left, right, d12 = source
    f = _fault(model_upload(right, left, d12))
    assert (f.array, f.row, f.n_bad) == ("x1", 0, N) and "exchanged" in f.hint, f
    # ... and for a part of the rows only
    x1, x2, d = _copy(clean)
    lo, hi = 2 * CHUNK - 1, 2 * CHUNK + 1
    x1[lo:hi], x2[lo:hi] = x2[lo:hi].copy(), x1[lo:hi].copy()
    f = _fault((x1, x2, d))
    assert (f.array, f.row, f.chunk, f.offset, f.n_bad) == ("x1", lo, 1, CHUNK - 1, 2) and "exchanged" in f.hint, f


def test_d1_and_d2_exchanged(source):
    left, right, d12 = source
    f = _fault(model_upload(left, right, d12[:, ::-1]))
    assert (f.array, f.row, f.n_bad) == ("d1", 0, N) and "d1 and d2 exchanged" in f.hint and "d2 of source row 0" in f.found, f


def test_one_permutation_of_all_arrays(source, clean):
    """What no reduction sees: the same rows exchanged in left, right and depths.  The sums stay what they were, bit for
    bit (every term is a multiple of 2^-24 and the totals stay below 2^53 of them)."""
    x1, x2, d = _copy(clean)
    a, b = CHUNK - 1, 2 * CHUNK + 5
    for arr in (x1, x2, d):
        arr[[a, b]] = arr[[b, a]]
    e, _ = restate((x1, x2, d))
    e0, _ = restate(clean)
    assert np.array_equal(e.sum(axis=0), e0.sum(axis=0)) and np.array_equal(d.sum(axis=0), source[2].sum(axis=0))
    assert np.array_equal(np.sort((e * e).sum(axis=1)), np.sort((e0 * e0).sum(axis=1)))     # the same squared norms, reordered
    f = up.first_fault(e, d, N, CHUNK)
    assert (f.array, f.row, f.chunk, f.offset, f.n_bad, f.last) == ("x1", a, 0, CHUNK - 1, 2, b) and f"row {b}" in f.found, f
    with pytest.raises(AssertionError, match="x1: first bad row"):
        up.check_rows(e, d, N, CHUNK, what="permuted")


def test_single_planes_and_values(clean):
    """Each array on its own: a stale, a zero, a duplicated row of one plane, and a residual that is merely rounded."""
    for which, name in enumerate(("x1", "x2", "d1", "d2")):
        x1, x2, d = _copy(clean)
        plane = (x1, x2, d[:, 0:1], d[:, 1:2])[which]
        plane[7] = plane[6]                          # duplicated
        plane[CHUNK + 3] = 0.0                       # zero
        f = _fault((x1, x2, d))
        assert (f.array, f.row, f.n_bad, f.last) == (name, 7, 2, CHUNK + 3) and "shifted by -1" in f.hint, (name, f)
    x1, x2, d = _copy(clean)
    x1[5, 2] = x1[4, 2]                              # only the z plane one row behind
    f = _fault((x1, x2, d))
    assert (f.array, f.row, f.n_bad) == ("x1", 5, 1), f
    e, d = restate(_copy(clean))
    e[11, 0] = np.nextafter(e[11, 0], 0.0)           # 1 ulp: below the bound, not bit-equal, and no code any more
    f = up.first_fault(e, d, N, CHUNK)
    assert f is not None and f.row == 11, f
