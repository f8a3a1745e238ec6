"""Row-identifying upload inputs and their decoder (plain numpy, test infrastructure).

Every upload path re-lays rows out in chunks; a row in the wrong slot is invisible to a reduction.  The inputs here make
every row of every array name itself, so that what comes back from the device says, row by row, which source row (of
which array) a plane holds.  For absolute row i < 2^24 = MAX_ROWS:

    left  (x1) row i:  ((i & 4095) + 1) / 4096,  ((i >> 12) + 1) / 4096,  ((i % 4093) + 1) / 4096    fractions in (0, 1]
    right (x2) row i:   (i & 4095) + 1,           (i >> 12) + 1,           (i % 4091) + 2             integers in [1, 4096]
    d1 of row i:        (i + 1) / 2^24                                                                 in (0, 1]
    d2 of row i:        1 + (i + 1) / 2^24                                                             in (1, 2]

All of them are exact in float32 (at most 13 significant bits for x, and the depth planes are always f64), so f32 planes
hold them unchanged.  With rot = tran = 0 and uniform depths 1 the residual is e = x2 - x1 (tests/test_gpu_residuals.py:
_reference with R = I), every component an integer minus a fraction of the 2^-12 grid: exact in float64.  Component k
lies in [A - 1, A) for the right code A, so A = floor(e) + 1 and the left code is (A - e) * 4096: one residual call
identifies the x1 row and the x2 row of every slot independently.  x and y carry the row, z carries it again modulo two
primes, so a z plane out of step with x and y is seen too.  The depths are read back as they are (a joint solve that may
not iterate hands the planes' depths out untouched); each column carries the whole row, and the two value ranges do not
meet, so d1 and d2 name themselves as well.  Zero is no code of any array: a slot never written is seen as such.

first_fault() names the first bad slot, its chunk and its offset within the chunk, what the slot holds instead and what
that points at; check_rows() asserts that there is none and that the residuals equal the long-double restatement under
the bound of tests/test_gpu_residuals.py (and, where asked, bit for bit)."""
from typing import NamedTuple

import numpy as np

GRID = 4096                  # codes per component
MAX_ROWS = 1 << 24           # rows the codes tell apart
ZL, ZR = 4093, 4091          # the z codes repeat with these periods (primes below GRID)
DEPTH_STEP = 2.0 ** -24
REL_TOL = 1e-12              # tests/test_gpu_residuals.py: |e - ref| <= REL_TOL * max(1, d1 + d2 + |t|)
SCALE = 2.0                  # max(1, d1 + d2 + |t|) at d1 = d2 = 1, t = 0
ARRAYS = ("x1", "x2", "d1", "d2")


def _rows(n, row0):
    if row0 < 0 or row0 + n > MAX_ROWS:
        raise ValueError(f"rows {row0} .. {row0 + n} are not all below {MAX_ROWS}")
    return np.arange(row0, row0 + n, dtype=np.int64)


def left_codes(i):
    i = np.asarray(i, dtype=np.int64)
    return np.stack([(i & 4095) + 1, (i >> 12) + 1, i % ZL + 1], axis=-1) / float(GRID)


def right_codes(i):
    i = np.asarray(i, dtype=np.int64)
    return np.stack([(i & 4095) + 1, (i >> 12) + 1, i % ZR + 2], axis=-1).astype(np.float64)


def depth_codes(i):
    i = np.asarray(i, dtype=np.int64)
    d1 = (i + 1) * DEPTH_STEP
    return np.stack([d1, 1.0 + d1], axis=-1)


def patterns(n, row0=0):
    """(left (n, 3), right (n, 3), d12 (n, 2)) of the absolute rows row0 .. row0 + n, float64 and C-contiguous."""
    i = _rows(n, row0)
    return left_codes(i), right_codes(i), depth_codes(i)


def reference_e(x1, x2):
    """The residual e = d2 x2 - (R (d1 x1) - t) at rot = tran = 0, d1 = d2 = 1, in long double: R = I, so x2 - x1."""
    return np.asarray(x2, dtype=np.longdouble) - np.asarray(x1, dtype=np.longdouble)


def _xy_row(cx, cy, cz, period, z0):
    """Row named by integer codes cx, cy in [1, 4096] and cz = row % period + z0; -1 where they name none."""
    ok = (cx >= 1) & (cx <= GRID) & (cy >= 1) & (cy <= GRID)
    row = np.where(ok, (cx - 1) + ((cy - 1) << 12), -1)
    ok &= cz == row % period + z0
    return np.where(ok, row, -1)


def decode_e(e):
    """(left_row, right_row), each (n,) int64: the source rows whose codes the residual e = x2 - x1 is made of; -1 where
    the three components are not the codes of one row."""
    e = np.asarray(e, dtype=np.float64).reshape(-1, 3)
    fin = np.isfinite(e).all(axis=1)
    ee = np.where(fin[:, None], e, 0.0)
    A = np.floor(ee) + 1.0                       # right code: e in [A - 1, A)
    a = (A - ee) * float(GRID)                   # left code, exact: a power-of-two scaling of an exact difference
    whole = (a == np.rint(a)).all(axis=1) & (np.abs(ee) < 2.0 * GRID).all(axis=1) & fin
    Ai, ai = A.astype(np.int64), np.rint(a).astype(np.int64)
    right = _xy_row(Ai[:, 0], Ai[:, 1], Ai[:, 2], ZR, 2)
    left = _xy_row(ai[:, 0], ai[:, 1], ai[:, 2], ZL, 1)
    return np.where(whole, left, -1), np.where(whole, right, -1)


def _code_row(x, scale, period, z0):
    """Row whose code triple x (n, 3) is (times scale: integers in [1, 4096]), -1 where it is none."""
    c = np.where(np.isfinite(x), x, 0.0) * scale
    ci = np.rint(np.clip(c, -1.0, 2.0 * GRID)).astype(np.int64)
    return np.where((c == ci).all(axis=1), _xy_row(ci[:, 0], ci[:, 1], ci[:, 2], period, z0), -1)


def left_row(x):
    return _code_row(np.asarray(x, dtype=np.float64).reshape(-1, 3), float(GRID), ZL, 1)


def right_row(x):
    return _code_row(np.asarray(x, dtype=np.float64).reshape(-1, 3), 1.0, ZR, 2)


def _is_code_value(v):
    """Is v a value that some uploaded array holds somewhere (or zero): what a stale or misdirected copy leaves behind."""
    depth_or_fraction = (v > 0.0) & (v <= 2.0) & (v / DEPTH_STEP == np.rint(v / DEPTH_STEP))
    return (v == 0.0) | depth_or_fraction | ((v >= 1.0) & (v <= GRID + 1.0) & (v == np.rint(v)))


def attribute(e, want):
    """(left_row, right_row, bad_x1, bad_x2) per slot.  A slot is bad exactly when decode_e does not give `want` for both
    sides: detection needs nothing more.  Where e decodes to two rows the sides are told apart by the decode itself.  Where
    it decodes to none (one plane holds something that is no row of its own array) each side is tried as the intact one:
    the other plane's value then follows from e.  The side is blamed whose implied value is another row of its own array;
    failing that, the only side whose implied components are values some uploaded array holds (stale data is made of
    those, an intact plane minus stale data is not); if that does not decide, both are."""
    left, right = decode_e(e)
    bad1, bad2 = left != want, right != want
    inv = np.flatnonzero((left < 0) & (right < 0))
    if inv.size:
        ei = np.where(np.isfinite(e[inv]), e[inv], 0.0)
        x1_if = right_codes(want[inv]) - ei              # x1 if x2 is intact
        x2_if = ei + left_codes(want[inv])               # x2 if x1 is intact
        l_if, r_if = left_row(x1_if), right_row(x2_if)
        same = ei == (right_codes(want[inv]) - left_codes(want[inv]))                   # components that are as expected
        p1, p2 = (_is_code_value(x1_if) | same).all(axis=1), (_is_code_value(x2_if) | same).all(axis=1)
        only1 = (l_if >= 0) | ((r_if < 0) & p1 & ~p2)
        only2 = ~only1 & ((r_if >= 0) | (p2 & ~p1))
        left[inv] = np.where(only1, l_if, left[inv])
        right[inv] = np.where(only2, r_if, right[inv])
        bad2[inv] = ~only1
        bad1[inv] = ~only2
    return left, right, bad1, bad2


def decode_depth(d):
    """(row, which) of one depth column: which = 1 for a d1 code, 2 for a d2 code, 0 (and row -1) for neither."""
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    fin = np.isfinite(d)
    dd = np.where(fin, d, 0.0)
    which = np.where(fin & (dd > 0.0) & (dd <= 1.0), 1, np.where(fin & (dd > 1.0) & (dd <= 2.0), 2, 0))
    k = np.where(which == 2, dd - 1.0, dd) / DEPTH_STEP
    ok = (which > 0) & (k == np.rint(k)) & (k >= 1)
    return np.where(ok, np.rint(k).astype(np.int64) - 1, -1), np.where(ok, which, 0)


class Fault(NamedTuple):
    array: str       # "x1", "x2", "d1", "d2", or "e" (the residual differs though every decoded row is right)
    row: int         # first bad slot, relative to the upload's first row
    chunk: int       # row // chunk
    offset: int      # row % chunk
    found: str       # what the slot holds
    hint: str        # the mechanism that would put it there
    n_bad: int       # bad slots of this array
    last: int        # last bad slot of this array

    def __str__(self):
        return (f"{self.array}: first bad row {self.row} = chunk {self.chunk} + {self.offset}; it holds {self.found}"
                f" -- {self.hint}; {self.n_bad} bad rows of {self.array}, the last at {self.last}")


def _hint(j, found_row, chunk, row0):
    """What puts absolute source row found_row into slot j (absolute row row0 + j)."""
    shift = found_row - (row0 + j)
    if abs(shift) < chunk and shift != 0:
        where = "from the start of its chunk on" if j % chunk == 0 else "inside a chunk"
        return f"source shifted by {shift:+d} rows {where}: a chunk's host source or its staging copy is off"
    if shift % chunk == 0:
        return (f"the row at the same offset of chunk {(found_row - row0) // chunk}: chunks exchanged, a stale staging "
                f"buffer, or a re-layout launched with another chunk's first row")
    return f"source row off by {shift:+d}: the destination index (first row + i, or the pair lookup) is wrong"


def _describe_x(which, j, e_row, found, chunk, row0):
    if found >= 0:
        return f"{which} of source row {found}", _hint(j, found, chunk, row0)
    if not np.isfinite(e_row).all():
        return f"a non-finite residual {e_row}", "uninitialised memory read"
    nl, nr = decode_e(-e_row[None])
    if nl[0] >= 0 and nr[0] >= 0:
        return (f"the negated residual of left row {nr[0]} and right row {nl[0]}",
                "left and right exchanged: each went into the other's planes")
    # one plane zero: e = x2 (left never written) or e = -x1 (right never written)
    if which == "x1" and np.array_equal(e_row, np.floor(e_row)) and (e_row >= 1).all():
        return "zero (e is x2 alone)", "never written: a chunk dropped, or written elsewhere"
    if which == "x2" and (e_row < 0).all() and (e_row >= -1).all():
        return "zero (e is -x1 alone)", "never written: a chunk dropped, or written elsewhere"
    if not e_row.any():
        return "zero, like the other side", "never written: a chunk dropped, or written elsewhere"
    return f"components of different rows or no code at all (e = {e_row.tolist()})", \
           "a copy that ends inside a row: a stale part of a copy thread's share, or a misaligned chunk boundary"


def _describe_d(col, j, value, found, kind, chunk, row0):
    if kind == col:
        return f"d{col} of source row {found}", _hint(j, found, chunk, row0)
    if kind != 0:
        return f"d{kind} of source row {found}", "d1 and d2 exchanged: the re-layout writes the columns to the wrong planes"
    if value == 0.0:
        return "zero", "never written: a chunk dropped, or written elsewhere"
    return f"{value!r}, no depth code", "a copy that ends inside a row, or depths that were modified"


def all_faults(e, d12, n, chunk, row0=0, bitwise=True):
    """The first bad slot of every array that has one (a list of Fault, in the order x1, x2, d1, d2, e).

    e: (n, 3) residuals read back at rot = tran = 0, d1 = d2 = 1; d12: (n, 2) depths read back, or None when none were
    uploaded; slot j must hold absolute source row row0 + j; chunk: rows per upload chunk (for the report)."""
    e = np.asarray(e, dtype=np.float64)
    if e.shape != (n, 3):
        raise AssertionError(f"residuals of shape {e.shape}, expected {(n, 3)}")
    want = _rows(n, row0)
    faults = []
    # the residual against the long-double restatement first: where it and the depths are right to the bit (the restatement
    # is exact in float64 for these codes, so that is error 0 under the bound) there is nothing to decode
    ref = reference_e(left_codes(want), right_codes(want))
    ref64 = ref.astype(np.float64)
    if d12 is not None and np.shape(d12) != (n, 2):
        raise AssertionError(f"depths of shape {np.shape(d12)}, expected {(n, 2)}")
    if np.array_equal(ref64.astype(np.longdouble), ref) and np.array_equal(e, ref64) and \
            (d12 is None or np.array_equal(np.asarray(d12, dtype=np.float64), depth_codes(want))):
        return faults

    def add(array, bad, describe):
        idx = np.flatnonzero(bad)
        if idx.size:
            j = int(idx[0])
            found, hint = describe(j)
            faults.append(Fault(array, j, j // chunk, j % chunk, found, hint, int(idx.size), int(idx[-1])))

    left, right, bad1, bad2 = attribute(e, want)
    add("x1", bad1, lambda j: _describe_x("x1", j, e[j], int(left[j]), chunk, row0))
    add("x2", bad2, lambda j: _describe_x("x2", j, e[j], int(right[j]), chunk, row0))
    if d12 is not None:
        d12 = np.asarray(d12, dtype=np.float64)
        if d12.shape != (n, 2):
            raise AssertionError(f"depths of shape {d12.shape}, expected {(n, 2)}")
        for col in (1, 2):
            rows, kind = decode_depth(d12[:, col - 1])
            add(f"d{col}", (rows != want) | (kind != col),
                lambda j, col=col, rows=rows, kind=kind: _describe_d(col, j, float(d12[j, col - 1]), int(rows[j]),
                                                                     int(kind[j]), chunk, row0))
    # the residual itself against the long-double restatement: the file's bound, and bit for bit where asked
    err = np.abs(e.astype(np.longdouble) - ref).max(axis=1) / SCALE
    bad = ~(err <= REL_TOL)
    if bitwise:
        bad |= (e != ref64).any(axis=1)
    add("e", bad, lambda j: (f"e = {e[j].tolist()} against {ref[j].astype(np.float64).tolist()}",
                             "every decoded row is right but the value is not: the residual arithmetic rounds"))
    return faults


def first_fault(e, d12, n, chunk, row0=0, bitwise=True):
    """The first slot (lowest row, then x1 < x2 < d1 < d2 < e) that does not hold its own source row, or None."""
    faults = all_faults(e, d12, n, chunk, row0=row0, bitwise=bitwise)
    if not faults:
        return None
    return min(faults, key=lambda f: (f.row, (ARRAYS + ("e",)).index(f.array)))


def check_rows(e, d12, n, chunk, row0=0, bitwise=True, what=""):
    f = first_fault(e, d12, n, chunk, row0=row0, bitwise=bitwise)
    assert f is None, f"{what}: {f}"
