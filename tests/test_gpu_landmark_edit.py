"""GPU: the edits of the landmark map (api.Landmarks: scores / prune / append / append_device / gather / gather_device) against the
numpy restatement of tests/landmark_edit_reference.py -- fancy indexing and concatenation of the handle's own downloaded state, and
the score in the product's order.  EVERY comparison is byte for byte: the edits move data and the score is exact by construction, so
there is no tolerance anywhere.  The maps are seeded as the fusion tests' and carry counts of 0, 1 and 2 from two real fuse passes
with a gate.  Sizes at the vector-per-lane, wave, block and tile edges and three tiles; four tiles with SBA_RESECT_GRID=1.  A dense
fuse after every kind of edit against a fresh handle set from the same rows shows the padding is zero.  Planted rows of every invalid
kind; the dry run; commutation with fuse; bytes across grids and histories; refusals; the incremental loop on the device against the
same route through host arrays."""
import ctypes as C

import numpy as np
import pytest

import landmark_edit_reference as le
import landmark_fusion_reference as lf
import resection_reference as rr
import resection_weighted_reference as wr
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100)
GRIDS = (None, "1", "2", "3", "5")
INF = float("inf")


def _state(L):
    X, Cv = L.get()
    return X, Cv, L.counts()


def _bytes(L):
    return le.state_bytes(_state(L))


def _build(L, n, planted=False):
    """The seeded map with its two frames fused: counts of 0, 1 and 2.  -> the first frame's bearings and the pose."""
    X, cov, frames, (rot, tran) = le.edit_map(n, planted)
    L.set(X, cov, le.COV_SCALE)
    for y, idx in frames:
        L.fuse(y, rot, tran, 1e-3, lf.GATE, idx=idx)
    return frames[0][0], rot, tran


def _record(p):
    return (p.n_before, p.n_invalid, p.n_uncertain, p.n_unobserved, p.n_masked, p.n_kept)


def _fuse_like_a_fresh_set(L, y, rot, tran):
    """A dense fuse on L gives the bytes, chi2 and counts of a fresh handle set from L's rows: nothing but zeros lies beyond n."""
    X, Cv, k = _state(L)
    with api.Landmarks(0) as T:
        T.set(X, Cv, 1.0)
        assert _bytes(T) == le.state_bytes((X, Cv, np.zeros(len(X), dtype=np.uint32)))
        a = L.fuse(y, rot, tran, 1e-3, lf.GATE)
        b = T.fuse(y, rot, tran, 1e-3, lf.GATE)
        assert (a.n_obs, a.n_skipped, a.n_behind, a.n_gated, a.n_fused) == (b.n_obs, b.n_skipped, b.n_behind, b.n_gated, b.n_fused)
        assert a.chi2.tobytes() == b.chi2.tobytes()
        X1, C1, k1 = _state(L)
        X2, C2, k2 = _state(T)
        assert X1.tobytes() == X2.tobytes() and C1.tobytes() == C2.tobytes() and np.array_equal(k1 - k, k2)
    return a


@pytest.mark.parametrize("n", le.SIZES)
def test_scores_equal_the_reference_bit_for_bit(n):
    with api.Landmarks(0) as L:
        for planted in ((False, True) if n >= 255 else (False,)):
            _build(L, n, planted)
            X, Cv, _ = _state(L)
            s = L.scores()
            assert s.shape == (n,) and s.tobytes() == le.scores(X, Cv).tobytes()
            if planted:
                assert np.isposinf(s[le.planted_rows(n)["X = 0"]]).all() and np.isnan(s[le.planted_rows(n)["NaN in X"]]).all()


def _prune_by_mask(n):
    parities = set()
    with api.Landmarks(0) as L:
        for name in le.MASKS:
            y, rot, tran = _build(L, n)
            before = _state(L)
            if n >= 255:
                assert before[2].max() == 2 and (before[2] == 0).any() and (before[2] == 1).any()
            m = le.mask(name, n)
            want = np.flatnonzero(m).astype(np.int64)
            p = L.prune(mask=m)
            assert _record(p) == (n, 0, 0, 0, n - len(want), len(want)), (name, _record(p))
            assert p.kept.dtype == np.int64 and np.array_equal(p.kept, want), name
            assert L.size == len(want) and _bytes(L) == le.state_bytes(le.take(before, want)), name
            parities.add(len(want) % 2)
            f = _fuse_like_a_fresh_set(L, y[want], rot, tran)
            assert f.n_obs == len(want)
    return parities


@pytest.mark.parametrize("n", le.SIZES)
def test_prune_by_mask_equals_indexing(n):
    parities = _prune_by_mask(n)
    if n >= 3:
        assert parities == {0, 1}


@pytest.mark.parametrize("n", le.LONG)
def test_prune_by_mask_over_several_grid_stride_steps(monkeypatch, n):
    monkeypatch.setenv("SBA_RESECT_GRID", "1")
    assert _prune_by_mask(n) == {0, 1}


def _cuts(state):
    X, Cv, k = state
    cut = le.median_cut(le.scores(X, Cv))
    half = le.mask("half", len(X))
    return cut, [dict(max_score=cut), dict(min_count=1), dict(min_count=2), dict(mask=half), dict(max_score=cut, min_count=1, mask=half),
                 dict(max_score=cut, min_count=2, mask=half), dict(max_score=0.0)]


@pytest.mark.parametrize("n,grid", [(257, None), (2049, None), (4097, None), (6145, "1")])
def test_prune_by_criteria_on_planted_rows(monkeypatch, n, grid):
    """The five class counts and `kept` are exact against the reference on the handle's own state; every landmark is in one class."""
    if grid:
        monkeypatch.setenv("SBA_RESECT_GRID", grid)
    seen = np.zeros(5, dtype=int)
    with api.Landmarks(0) as L:
        _build(L, n, planted=True)
        first = _state(L)
        cut, cuts = _cuts(first)
        assert le.margin_ok(le.scores(first[0], first[1]), cut)            # as tests/test_landmark_edit_host_cpu.py qualifies it
        for k, kw in enumerate(cuts):
            if k:
                _build(L, n, planted=True)
            before = _state(L)
            assert le.state_bytes(before) == le.state_bytes(first)
            want, record = le.prune(*before, **kw)
            p = L.prune(**kw)
            assert _record(p) == record and sum(record[1:]) == n, (kw.keys(), _record(p), record)
            assert np.array_equal(p.kept, want)
            assert L.size == len(want) and _bytes(L) == le.state_bytes(le.take(before, want))
            seen += np.array(record[1:])
            assert record[1] >= 8                                          # the planted NaN and inf rows at least
        assert (seen > 0).all()
        rows = le.planted_rows(n)
        cls = le.classify(*first)
        assert all(cls[i] == le.INVALID for name in ("NaN in X", "inf in Sigma") for i in rows[name]) and (cls[rows["X = 0"]] == le.KEPT).all()
        assert (le.classify(*first, max_score=1e300)[rows["X = 0"]] == le.UNCERTAIN).all()


def test_a_dry_run_reports_the_same_and_changes_nothing():
    n = 4097
    with api.Landmarks(0) as L, api.Landmarks(0) as T:
        for H in (L, T):
            _build(H, n, planted=True)
        before = _bytes(L)
        cut, cuts = _cuts(_state(L))
        for kw in cuts[4:6]:
            dry = L.prune(apply=False, **kw)
            assert _bytes(L) == before and L.size == n
            bare = L.prune(apply=False, want_kept=False, **kw)
            assert _bytes(L) == before and bare.kept is None and _record(bare) == _record(dry)
            wet = T.prune(**kw)
            assert _record(dry) == _record(wet) and np.array_equal(dry.kept, wet.kept) and 0 < wet.n_kept < n
            assert T.prune(want_kept=False).n_kept == wet.n_kept       # a second prune of nothing: every survivor is kept
            _build(T, n, planted=True)
        assert L.prune(**cuts[4]).n_kept == L.size


def test_pruning_to_nothing_leaves_a_usable_empty_map():
    with api.Landmarks(0) as L:
        y, rot, tran = _build(L, 257)
        p = L.prune(mask=np.zeros(257, dtype=bool))
        assert _record(p) == (257, 0, 0, 0, 257, 0) and p.kept.shape == (0,) and L.size == 0
        assert L.get()[0].shape == (0, 3) and L.counts().shape == (0,) and L.scores().shape == (0,)
        assert _record(L.prune()) == (0, 0, 0, 0, 0, 0)
        Xa, Ca = le.extra_rows(513)
        L.append(Xa, Ca, 1.3)
        assert _bytes(L) == le.state_bytes((Xa, 1.3 * Ca, np.zeros(513, dtype=np.uint32)))


def _device_rows(Xa, Ca):
    """The rows on the device at 16-byte aligned addresses with NaN guard doubles around them -> (tensors, xyz ptr, cov ptr)."""
    import torch
    dev = torch.device("cuda", 0)
    gx = np.full(3 * len(Xa) + 4, np.nan)
    gc = np.full(6 * len(Ca) + 4, np.nan)
    gx[2:2 + 3 * len(Xa)] = Xa.reshape(-1)
    gc[2:2 + 6 * len(Ca)] = Ca.reshape(-1)
    tx, tc = torch.from_numpy(gx).to(dev), torch.from_numpy(gc).to(dev)
    torch.cuda.synchronize()
    assert tx.data_ptr() % 16 == 0 and tc.data_ptr() % 16 == 0
    return (tx, tc), tx.data_ptr() + 16, tc.data_ptr() + 16


@pytest.mark.parametrize("n0", (0, 1, 2, 2049))
def test_append_equals_concatenation(n0):
    with api.Landmarks(0) as L, api.Landmarks(0) as D:
        for n_add in (0, 1, 2, 513):
            Xa, Ca = le.extra_rows(n_add)
            for H in (L, D):
                y, rot, tran = _build(H, n0)
            before = _state(L)
            want = le.append(before, Xa, Ca, 1.3)
            L.append(Xa, Ca, 1.3)
            keep, px, pc = _device_rows(Xa, Ca)
            D.append_device(px, pc, n_add, 1.3)
            for H in (L, D):
                assert H.size == n0 + n_add and _bytes(H) == le.state_bytes(want), (n0, n_add)
            got = _state(L)
            assert le.state_bytes(tuple(a[:n0] for a in got)) == le.state_bytes(before) and not got[2][n0:].any()
            if n0 == 0:                                                    # onto an empty map: set
                with api.Landmarks(0) as T:
                    T.set(Xa, Ca, 1.3)
                    assert _bytes(T) == _bytes(L)
            ya = np.concatenate([y, lf.scene(max(n_add, 3), "closed").y[:n_add]])
            _fuse_like_a_fresh_set(L, ya, rot, tran)
            del keep


def test_appending_twice_equals_appending_the_concatenation():
    Xa, Ca = le.extra_rows(513)
    for n0, cut in ((1, 1), (2049, 256), (2, 511)):
        with api.Landmarks(0) as L, api.Landmarks(0) as T:
            for H in (L, T):
                _build(H, n0)
            L.append(Xa[:cut], Ca[:cut], 1.3)
            L.append(Xa[cut:], Ca[cut:], 1.3)
            T.append(Xa, Ca, 1.3)
            assert L.size == n0 + 513 and _bytes(L) == _bytes(T)


@pytest.mark.parametrize("n", (1, 3, 257, 4097))
def test_gather_equals_indexing(n):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31 + n)
    with api.Landmarks(0) as L:
        _build(L, n, planted=n >= 255)
        X, Cv, k = _state(L)
        before = _bytes(L)
        sub = lf.subset(n) if n > 3 else np.arange(n, dtype=np.int64)
        for idx in (sub, sub[::-1].copy(), rng.integers(0, n, size=2 * n + 5), np.arange(n), np.zeros(0, dtype=np.int64), np.full(67, n - 1)):
            idx = np.asarray(idx, dtype=np.int64)
            m = len(idx)
            gx, gc, gk = L.gather(idx)
            assert gx.shape == (m, 3) and gc.shape == (m, 6) and gk.dtype == np.uint32
            assert le.state_bytes((gx, gc, gk)) == le.state_bytes((X[idx], Cv[idx], k[idx]))
            ox = torch.full((3 * m + 4,), -7.0, dtype=torch.float64, device=dev)
            oc = torch.full((6 * m + 4,), -7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            L.gather_device(idx, ox.data_ptr() + 16, oc.data_ptr() + 16)
            hx, hc = ox.cpu().numpy(), oc.cpu().numpy()
            assert hx[2:2 + 3 * m].tobytes() == X[idx].tobytes() and hc[2:2 + 6 * m].tobytes() == Cv[idx].tobytes()
            assert (hx[:2] == -7.0).all() and (hx[2 + 3 * m:] == -7.0).all() and (hc[:2] == -7.0).all() and (hc[2 + 6 * m:] == -7.0).all()
            L.gather_device(idx, 0, oc.data_ptr())                         # either output may be skipped
            L.gather_device(idx, ox.data_ptr(), None)
        # the raw entry point: any host output may be NULL, and exactly m rows are written
        lib, h = L._lib, L._h
        idx = np.ascontiguousarray(sub[:max(1, len(sub) // 2)])
        m = len(idx)
        gc = np.full(6 * m + 2, -7.0)
        gk = np.full(m + 2, 77, dtype=np.uint32)
        ip = idx.ctypes.data_as(C.POINTER(C.c_int64))
        assert lib.sba_landmarks_gather(h, ip, m, None, gc.ctypes.data_as(cabi._dp), None) == cabi.SBA_OK
        assert lib.sba_landmarks_gather(h, ip, m, None, None, gk.ctypes.data_as(C.POINTER(C.c_uint32))) == cabi.SBA_OK
        assert gc[:6 * m].tobytes() == Cv[idx].tobytes() and (gc[6 * m:] == -7.0).all()
        assert np.array_equal(gk[:m], k[idx]) and (gk[m:] == 77).all()
        assert _bytes(L) == before


def test_prune_commutes_with_fuse():
    n = 4097
    X, cov, frames, (rot, tran) = le.edit_map(n)
    m = le.mask("half", n)
    idx = lf.subset(n)[::2].copy()                                         # the observed landmarks of a third frame
    y3 = frames[0][0][idx] * 1.5
    with api.Landmarks(0) as L, api.Landmarks(0) as T:
        for H in (L, T):
            _build(H, n)
        # prune, then fuse the observations that survived at their new rows
        p = L.prune(mask=m)
        new_row = np.full(n, -1, dtype=np.int64)
        new_row[p.kept] = np.arange(len(p.kept))
        seen = new_row[idx] >= 0
        a = L.fuse(y3[seen], rot, tran, 1e-3, lf.GATE, lf.POSE_COV_FULL, idx=new_row[idx][seen])
        # fuse, then prune
        b = T.fuse(y3, rot, tran, 1e-3, lf.GATE, lf.POSE_COV_FULL, idx=idx)
        q = T.prune(mask=m)
        assert np.array_equal(p.kept, q.kept) and _bytes(L) == _bytes(T)
        assert a.chi2.tobytes() == b.chi2[seen].tobytes() and 0 < a.n_fused < b.n_fused and a.n_obs == int(seen.sum())


def _cycle(L, n=4097):
    """Every edit once, on one handle -> the bytes of everything it returned and left behind, step by step, and the same by the
    reference for every step but the fuse (entry 5 of the first list)."""
    got, want = [], []
    y, rot, tran = _build(L, n, planted=True)
    ref = _state(L)
    s = L.scores()
    got.append(s.tobytes()); want.append(le.scores(ref[0], ref[1]).tobytes())
    cut = le.median_cut(s)
    half = le.mask("half", n)
    # prune -> append -> prune
    kept, record = le.prune(*ref, max_score=cut, min_count=1, mask=half)
    p = L.prune(cut, 1, half, apply=False)
    got.append(p.kept.tobytes() + np.array(_record(p)).tobytes()); want.append(kept.tobytes() + np.array(record).tobytes())
    p = L.prune(cut, 1, half)
    ref = le.take(ref, kept)
    got.append(p.kept.tobytes() + np.array(_record(p)).tobytes() + _bytes(L)); want.append(kept.tobytes() + np.array(record).tobytes() + le.state_bytes(ref))
    Xa, Ca = le.extra_rows(2049)
    L.append(Xa, Ca, 1.3)
    ref = le.append(ref, Xa, Ca, 1.3)
    got.append(_bytes(L)); want.append(le.state_bytes(ref))
    idx = np.arange(len(ref[0]) - 1, -1, -3, dtype=np.int64)
    got.append(le.state_bytes(L.gather(idx))); want.append(le.state_bytes(le.take(ref, idx)))
    f = L.fuse(np.concatenate([y[kept], lf.scene(2049, "closed").y]), rot, tran, 1e-3, lf.GATE)
    got.append(f.chi2.tobytes() + _bytes(L))
    ref = _state(L)
    kept, record = le.prune(*ref, min_count=1)
    p = L.prune(min_count=1)
    ref = le.take(ref, kept)
    got.append(p.kept.tobytes() + np.array(_record(p)).tobytes() + _bytes(L)); want.append(kept.tobytes() + np.array(record).tobytes() + le.state_bytes(ref))
    assert 0 < record[3] and 0 < record[5] < record[0]
    return got, want


def test_bytes_do_not_depend_on_the_grid_or_the_history(monkeypatch):
    seen = []
    for grid in GRIDS:
        if grid is None:
            monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
        else:
            monkeypatch.setenv("SBA_RESECT_GRID", grid)
        with api.Landmarks(0) as L:
            got, want = _cycle(L)
            assert len(got) == 7 and got[:5] + got[6:] == want             # against the reference cycle
            seen.append(b"".join(got))
            if grid in (None, "2"):
                seen.append(b"".join(_cycle(L)[0]))                        # the same again on the used handle: both buffers reused
    monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
    with api.Landmarks(0) as L:
        _build(L, 6145)                                                    # another, larger map, a prune and an append first
        L.prune(mask=le.mask("alternating", 6145))
        L.append(*le.extra_rows(513), 1.0)
        L.prune(min_count=2)
        seen.append(b"".join(_cycle(L)[0]))
    assert all(b == seen[0] for b in seen) and len(seen) == len(GRIDS) + 3


def _refused(code, calls):
    for name, call in calls.items():
        with pytest.raises(api.SbaError) as ei:
            call()
        assert ei.value.code == code and ei.value.message, name


def test_refusals_return_their_code_and_leave_the_map_alone():
    import torch
    n = 257
    Xa, Ca = le.extra_rows(5)
    with api.Landmarks(0) as L:
        _build(L, n)
        before = _bytes(L)
        t = torch.zeros(9 * n + 4, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ok = np.arange(5, dtype=np.int64)
        _refused(cabi.SBA_ERR_INVALID_ARG, {
            "NaN max_score": lambda: L.prune(max_score=np.nan), "negative max_score": lambda: L.prune(max_score=-1e-9),
            "-inf max_score": lambda: L.prune(max_score=-np.inf),
            "bad cov_scale": lambda: L.append(Xa, Ca, 0.0), "NaN cov_scale": lambda: L.append(Xa, Ca, np.nan),
            "infinite cov_scale": lambda: L.append_device(t.data_ptr(), t.data_ptr() + 64, 5, np.inf),
            "misaligned append": lambda: L.append_device(t.data_ptr() + 8, t.data_ptr() + 64, 5),
            "misaligned append cov": lambda: L.append_device(t.data_ptr(), t.data_ptr() + 24, 5),
            "null append": lambda: L.append_device(0, t.data_ptr(), 5),
            "too many rows": lambda: L.append_device(t.data_ptr(), t.data_ptr(), 2 ** 62),
            "idx == n": lambda: L.gather(np.array([0, n, 3])), "idx negative": lambda: L.gather(np.array([0, -1, 3])),
            "idx far out": lambda: L.gather(np.array([2 ** 62])),
            "idx == n to the device": lambda: L.gather_device(np.array([0, n]), t.data_ptr(), t.data_ptr() + 64),
            "misaligned gather": lambda: L.gather_device(ok, t.data_ptr() + 8, t.data_ptr() + 64),
        })
        # the raw entry points: NULL required pointers, nothing written
        lib, h = L._lib, L._h
        opt = cabi.LandmarkPruneOptions(INF, 0, None, 1)
        res = cabi.LandmarkPruneResult(-7, -7, -7, -7, -7, -7)
        rows = np.full(30, -7.0)
        dp = rows.ctypes.data_as(cabi._dp)
        assert lib.sba_landmarks_prune(h, None, C.byref(res), None) == cabi.SBA_ERR_INVALID_ARG and cabi.last_error(lib)
        assert lib.sba_landmarks_prune(h, C.byref(opt), None, None) == cabi.SBA_ERR_INVALID_ARG and cabi.last_error(lib)
        assert lib.sba_landmarks_scores(h, None) == cabi.SBA_ERR_INVALID_ARG and cabi.last_error(lib)
        assert lib.sba_landmarks_append(h, None, dp, 2, 1.0) == cabi.SBA_ERR_INVALID_ARG and cabi.last_error(lib)
        assert lib.sba_landmarks_append(h, dp, None, 2, 1.0) == cabi.SBA_ERR_INVALID_ARG and cabi.last_error(lib)
        assert lib.sba_landmarks_gather(h, None, 2, dp, dp, None) == cabi.SBA_ERR_INVALID_ARG and cabi.last_error(lib)
        bad = cabi.LandmarkPruneOptions(float("nan"), 0, None, 1)
        assert lib.sba_landmarks_prune(h, C.byref(bad), C.byref(res), None) == cabi.SBA_ERR_INVALID_ARG
        assert res.n_before == -7 and res.n_kept == -7 and (rows == -7.0).all()
        with pytest.raises(ValueError):
            L.prune(mask=np.ones(n + 1, dtype=bool))
        assert _bytes(L) == before and L.size == n                         # every refusal left the map alone
        L.append(Xa, Ca, 1.3)                                              # and the handle usable
        assert L.prune(min_count=1, want_kept=False).n_before == n + 5
        assert L.gather(ok)[0].shape == (5, 3)


def test_the_incremental_loop_on_the_device_equals_the_route_through_host_arrays():
    """A solved pair's structure_joint_into -> set_device; gather_device(idx) -> Problem.upload_device + set_landmark_covariances_device
    -> solve_resection_weighted -> resection_covariance -> fuse(idx, pose_cov); append_device of a second pair's structure;
    prune(max_score, min_count).  Byte-identical to the same route through host arrays and numpy."""
    import torch
    n, n2 = 513, 257
    f, f2 = rr.three_frames(n, 71), rr.three_frames(n2, 72)
    opt = api.default_lm_options(tran_param=api.TRAN_SPHERE, **TIGHT)
    lm = api.default_lm_options(huber_delta=wr.DELTA, **TIGHT)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    dev = torch.device("cuda", 0)
    idx = lf.subset(n)
    m = len(idx)

    def solved(p, g):
        factor = np.linalg.norm(g.tran_ab)
        p.upload(g.x1, g.x2, g.d12 / factor * 1.01)
        t0 = g.tran_ab / factor + 0.02 * axis
        rot, tran, _, _ = p.solve_joint(g.rot_ab + 0.02 * axis, t0 / np.linalg.norm(t0), options=opt)
        return rot, tran

    with api.Problem(0) as p, api.Problem(0) as p2, api.Problem(0) as q, api.Problem(0) as q2, api.Landmarks(0) as L, api.Landmarks(0) as L2:
        rot, tran = solved(p, f)
        rot2, tran2 = solved(p2, f2)
        tx = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        tc = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        ax = torch.zeros((n2, 3), dtype=torch.float64, device=dev)
        ac = torch.zeros((n2, 6), dtype=torch.float64, device=dev)
        ox = torch.zeros((m, 3), dtype=torch.float64, device=dev)
        oc = torch.zeros((m, 6), dtype=torch.float64, device=dev)
        gy = torch.from_numpy(np.ascontiguousarray(f.y[idx])).to(dev)
        ones = torch.ones((m, 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        # on the device
        pose = p.structure_joint_into(tx.data_ptr(), tc.data_ptr(), None, rot, tran, options=opt)
        scale = max(pose.sigma2, 1e-6)
        L.set_device(tx.data_ptr(), tc.data_ptr(), n, scale)
        L.gather_device(idx, ox.data_ptr(), oc.data_ptr())
        q.upload_device(ox.data_ptr(), gy.data_ptr(), ones.data_ptr(), m)
        q.set_landmark_covariances_device(oc.data_ptr(), 1.0)
        g = q.resection_guess()
        r, t, _, nb = q.solve_resection_weighted(g.rot, g.tran, lm, bearing_sigma=1e-3, reweight_rounds=2)
        cv = q.resection_covariance(r, t, lm)
        fd = L.fuse(f.y[idx], r, t, 1e-3, lf.GATE, cv.cov, idx=idx)
        pose2 = p2.structure_joint_into(ax.data_ptr(), ac.data_ptr(), None, rot2, tran2, options=opt)
        scale2 = max(pose2.sigma2, 1e-6)
        L.append_device(ax.data_ptr(), ac.data_ptr(), n2, scale2)
        cut = le.median_cut(L.scores())
        pd = L.prune(cut, 1)
        # through host arrays and numpy
        st = p.structure_joint(rot, tran, options=opt)
        L2.set(st.xyz, st.cov, scale)
        Xg, Cg, _ = L2.gather(idx)
        q2.upload(Xg, f.y[idx], np.ones((m, 2)))
        q2.set_landmark_covariances(Cg, 1.0)
        g2 = q2.resection_guess()
        r2, t2, _, nb2 = q2.solve_resection_weighted(g2.rot, g2.tran, lm, bearing_sigma=1e-3, reweight_rounds=2)
        cv2 = q2.resection_covariance(r2, t2, lm)
        assert r2.tobytes() == r.tobytes() and t2.tobytes() == t.tobytes() and cv2.cov.tobytes() == cv.cov.tobytes() and nb == nb2 == 0
        fh = L2.fuse(f.y[idx], r2, t2, 1e-3, lf.GATE, cv2.cov, idx=idx)
        assert fh.chi2.tobytes() == fd.chi2.tobytes() and fh.n_fused == fd.n_fused and fd.n_fused > m // 2
        st2 = p2.structure_joint(rot2, tran2, options=opt)
        host = le.append(_state(L2), st2.xyz, st2.cov, scale2)
        assert np.isfinite(host[0]).all() and np.isfinite(host[1]).all()
        assert le.median_cut(le.scores(host[0], host[1])) == cut and le.margin_ok(le.scores(host[0], host[1]), cut)
        kept, record = le.prune(*host, max_score=cut, min_count=1)
        assert _record(pd) == record and np.array_equal(pd.kept, kept)
        assert _bytes(L) == le.state_bytes(le.take(host, kept))
        # the appended landmarks have no observation yet: each of them is uncertain or unobserved, none is kept
        assert record[2] > 0 and record[3] > 0 and record[2] + record[3] >= n2 and 0 < record[5] <= fd.n_fused and kept.max() < n
