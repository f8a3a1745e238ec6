"""GPU: the landmark map's descriptor rows and the association of a frame with the map, byte for byte
against tests/landmark_associate_reference.py -- no tolerance anywhere: integer-valued descriptors inside
match_cases.assert_exact_domain make every f32 operation of the path exact.  The host and the _device forms both; the planted
cases of the reference's table, permutations (no contest), pools of exact copies (nearly nothing passes the ratio test), the
inclusive distance cut, the degenerate sizes, strided layouts; the descriptors through set / get / prune / append / set again
against numpy indexing; an undescribed map as before; histories, grids and runs; and the chain the feature exists for:
associate_device -> register_robust_device equals register_robust fed the reference's idx and host-gathered bearings."""
import numpy as np
import pytest

import landmark_associate_reference as la
import landmark_register_robust_reference as rb
import match_cases as mc
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

TILE = mc.compact_tile()
TIGHT = dict(function_tolerance=1e-30, parameter_tolerance=1e-13, gradient_tolerance=1e-13, max_num_iterations=100)


def _map(L, desc, seed=0):
    xyz, cov = la.map_rows(len(desc), seed)
    L.set(xyz, cov)
    L.set_descriptors(desc)
    return xyz, cov


def _bytes(a, bearings=None):
    b = getattr(a, "bearings", None) if bearings is None else bearings
    return (repr((a.n_frame, a.n_accepted, a.n_contested, a.n_associated)).encode() + np.ascontiguousarray(a.idx, dtype=np.int64).tobytes()
            + np.ascontiguousarray(a.rows, dtype=np.int32).tobytes() + np.ascontiguousarray(a.distance, dtype=np.float32).tobytes()
            + (b"" if b is None else np.ascontiguousarray(b, dtype=np.float64).tobytes()))


def _want(ref, y=None):
    return _bytes(ref, None if y is None else y[ref.rows])


def _device_form(L, frame, y, layout="contig", **kw):
    """associate_device on torch copies of the frame: (LandmarkAssociation, gathered bearings from the device buffer), and the
    guard rows of that buffer behind the associated ones untouched."""
    import torch
    dev = torch.device("cuda:0")
    wide = mc.strided(frame, layout)
    pad = mc.LAYOUTS[layout][0]
    m, dim = frame.shape
    base = wide.base if pad else wide
    f_dev = torch.from_numpy(np.array(base)).to(dev)
    y_dev = torch.from_numpy(np.array(y)).to(dev) if y is not None else None
    cap = min(L.size, m)
    out = torch.full((3 * cap + 4,), -7.0, dtype=torch.float64, device=dev)
    assert out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    got = L.associate_device(f_dev.data_ptr(), m, dim, None if y is None else y_dev.data_ptr(), None if y is None else out.data_ptr(),
                             row_stride_bytes=4 * (dim + pad), **kw)
    torch.cuda.synchronize()
    flat = out.cpu().numpy()
    k = got.n_associated if y is not None else 0
    assert (flat[3 * k:] == -7.0).all()
    assert torch.equal(f_dev.cpu().view(torch.int32), torch.from_numpy(np.array(base)).view(torch.int32))     # the caller's rows are only read
    return got, (flat[:3 * k].reshape(-1, 3).copy() if y is not None else None)


def _both_forms(L, frame, y, ref, tag, **kw):
    want = _want(ref, y)
    host = L.associate(frame, y, **kw)
    assert _bytes(host) == want, (tag, "host", (host.n_accepted, host.n_associated, host.n_contested), (ref.n_accepted, ref.n_associated, ref.n_contested))
    got, gathered = _device_form(L, frame, y, **kw)
    assert _bytes(got, gathered) == want, (tag, "device")
    assert (np.diff(host.idx) > 0).all() and len(set(host.rows.tolist())) == len(host.rows)
    assert host.n_accepted == host.n_contested + host.n_associated


# ---- 1. the planted cases of the table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(la.CASES)))
def test_planted_cases_against_the_reference(k):
    frame, desc = la.arrays(k)
    y = la.bearings_for(len(frame), k)
    with api.Landmarks(0) as L:
        _map(L, desc, k)
        state = L.get_descriptors().tobytes()
        for ratio in la.RATIOS:
            ref = la.expected(k, ratio)
            assert (ref.n_accepted, ref.n_associated, ref.n_contested) == la.CASES[k].counts[ratio]
            _both_forms(L, frame, y, ref, (k, ratio), ratio=ratio)
        # without bearings: the same idx, rows and distances, and nothing gathered
        bare = L.associate(frame, ratio=0.3)
        assert bare.bearings is None and _bytes(bare) == _want(la.expected(k, 0.3))
        assert L.get_descriptors().tobytes() == state == desc.tobytes()        # an association only reads the map


def test_permutations_have_no_contest():
    for nq, nt, D in ((256, 8193, 64), (129, 129, 200)):
        frame, desc = mc.perm_pair(nq, nt, D)
        with api.Landmarks(0) as L:
            _map(L, desc)
            ref = la.associate(frame, desc, 0.3)
            got = L.associate(frame, la.bearings_for(nq), ratio=0.3)
            assert got.n_contested == 0 and got.n_accepted == got.n_associated == nq
            assert np.array_equal(got.idx, np.sort(mc.perm_of(nq, nt, D))) and (got.distance == 0.0).all()
            _both_forms(L, frame, la.bearings_for(nq), ref, (nq, nt, D), ratio=0.3)


def test_pools_of_exact_copies_count_exactly():
    """Exact copies everywhere: d0 = d1 = 0 fails every ratio, so nothing (D = 64) or nearly nothing (D = 200: two rows, one
    landmark, contested) is accepted, and the counts are still the reference's."""
    accepted = []
    for nq, nt, D in ((257, 2049, 64), (257, 2049, 200)):
        frame, desc = mc.ties_pool_pair(nq, nt, D)
        with api.Landmarks(0) as L:
            _map(L, desc)
            for ratio in (0.3, 1.0, 1.5):
                ref = la.associate(frame, desc, ratio)
                _both_forms(L, frame, la.bearings_for(nq), ref, (D, ratio), ratio=ratio)
                accepted.append(ref.n_accepted)
    assert max(accepted) < 257 // 8 and accepted[:3] == [0, 0, 0] and accepted[3:] == [2, 2, 2]


def test_the_distance_cut_is_inclusive():
    frame, desc = la.arrays(0)
    y = la.bearings_for(len(frame))
    with api.Landmarks(0) as L:
        _map(L, desc)
        ref = la.expected(0, 0.3, 1.0)
        everything = la.expected(0, 0.3)
        assert 0 < ref.n_accepted < everything.n_accepted and (ref.distance == 1.0).all() and (everything.distance > 1.0).any()
        _both_forms(L, frame, y, ref, "max_distance 1", ratio=0.3, max_distance=1.0)
        below = la.associate(frame, desc, 0.3, np.nextafter(np.float32(1.0), np.float32(0.0)))
        assert below.n_accepted == 0
        _both_forms(L, frame, y, below, "just below 1", ratio=0.3, max_distance=float(np.nextafter(np.float32(1.0), np.float32(0.0))))


# ---- 2. degenerate sizes, NaN rows, strided layouts --------------------------------------------------------------------------------
def test_degenerate_sizes_give_zeros():
    frame, desc = la.arrays(4)
    with api.Landmarks(0) as L:
        for n in (0, 1):
            _map(L, desc[:n])
            assert L.size == n and L.descriptor_dim == desc.shape[1]
            got = L.associate(frame, la.bearings_for(len(frame)))
            assert (got.n_frame, got.n_accepted, got.n_contested, got.n_associated) == (len(frame), 0, 0, 0) and got.idx.size == 0
            dev, gathered = _device_form(L, frame, la.bearings_for(len(frame)))
            assert _bytes(dev, gathered) == _bytes(got)
        _map(L, desc)
        got = L.associate(frame[:0], np.zeros((0, 3)))
        assert (got.n_frame, got.n_accepted, got.n_contested, got.n_associated) == (0, 0, 0, 0) and got.rows.size == 0


def test_a_frame_row_with_a_nan_matches_nothing():
    frame, desc = la.arrays(2)
    frame = np.array(frame)
    ref0 = la.expected(2, 0.5)
    victim = int(ref0.rows[3])                                  # a winner: its landmark goes to the next claimant
    frame[victim, 1] = np.nan
    frame[5, 0] = np.inf
    ref = la.associate(frame, desc, 0.5)
    assert victim not in ref.rows and 5 not in ref.rows and ref.n_accepted == ref0.n_accepted - 2
    with api.Landmarks(0) as L:
        _map(L, desc)
        _both_forms(L, frame, la.bearings_for(len(frame)), ref, "nan row", ratio=0.5)


@pytest.mark.parametrize("layout", [name for name in mc.LAYOUTS if name != "contig"])
def test_strided_layouts_on_both_sides(layout):
    k = 0 if mc.LAYOUTS[layout][0] == 1 else 3
    frame, desc = la.arrays(k)
    y = la.bearings_for(len(frame))
    ref = la.expected(k, 0.3)
    with api.Landmarks(0) as L:
        xyz, cov = la.map_rows(len(desc))
        L.set(xyz, cov)
        L.set_descriptors(mc.strided(desc, layout))                    # the map's rows from a padded view
        assert L.get_descriptors().tobytes() == desc.tobytes()
        host = L.associate(mc.strided(frame, layout), y, ratio=0.3)
        assert _bytes(host) == _want(ref, y), layout
        got, gathered = _device_form(L, frame, y, layout=layout, ratio=0.3)
        assert _bytes(got, gathered) == _want(ref, y), layout


# ---- 3. the descriptors through the map's life ---------------------------------------------------------------------------------------
def _any_bits(n, dim, seed):
    """(n, dim) float32 of arbitrary bit patterns (NaN payloads, denormals, both zeros): the moves are copies of bytes."""
    return np.random.default_rng([79, n, dim, seed]).integers(0, 2**32, size=(n, dim), dtype=np.uint32).view(np.float32)


def _state(L):
    X, Cv = L.get()
    return X.tobytes() + Cv.tobytes() + L.counts().tobytes()


@pytest.mark.parametrize("n,dim", ((TILE - 1, 36), (TILE, 5), (TILE + 1, 64), (2 * TILE + 3, 256), (301, 200), (300, 1)))
def test_set_get_and_prune_against_numpy_indexing(n, dim):
    desc = _any_bits(n, dim, 0)
    rng = np.random.default_rng([80, n, dim])
    with api.Landmarks(0) as L:
        xyz, cov = _map(L, desc)
        assert L.descriptor_dim == dim and L.get_descriptors().tobytes() == desc.tobytes()
        pick = rng.integers(0, n, size=n // 3 + 7)
        pick[:3] = (n - 1, 0, n - 1)                                 # any order, repeats
        assert L.get_descriptors(pick).tobytes() == desc[pick].tobytes()
        assert L.get_descriptors(np.zeros(0, dtype=np.int64)).shape == (0, dim)
        mask = rng.random(n) < 0.6
        mask[[0, n - 1]] = (True, False)
        before = _state(L)
        dry = L.prune(mask=mask, apply=False)
        assert np.array_equal(dry.kept, np.flatnonzero(mask)) and L.size == n and _state(L) == before
        assert L.get_descriptors().tobytes() == desc.tobytes()              # a dry run moves nothing
        res = L.prune(mask=mask)
        kept = np.flatnonzero(mask)
        assert np.array_equal(res.kept, kept) and (res.n_before, res.n_masked, res.n_kept) == (n, n - len(kept), len(kept))
        assert L.get_descriptors().tobytes() == desc[kept].tobytes() and L.descriptor_dim == dim
        X, Cv = L.get()
        assert X.tobytes() == xyz[kept].tobytes() and Cv.tobytes() == cov[kept].tobytes() and not L.counts().any()
        # a second prune from the swapped allocations, then to empty: the dimension stays
        mask2 = rng.random(len(kept)) < 0.5
        L.prune(mask=mask2)
        assert L.get_descriptors().tobytes() == desc[kept][mask2].tobytes()
        L.prune(mask=np.zeros(L.size, dtype=bool))
        assert L.size == 0 and L.descriptor_dim == dim and L.get_descriptors().shape == (0, dim)
        # a replacement of another dimension, and the drop
        xyz, cov = _map(L, _any_bits(9, 7, 1))
        assert L.descriptor_dim == 7 and L.get_descriptors().tobytes() == _any_bits(9, 7, 1).tobytes()
        L.set_descriptors(None)
        assert L.descriptor_dim == 0 and L.size == 9
        with pytest.raises(cabi.SbaError):
            L.get_descriptors()


def test_append_keeps_the_rows_in_step():
    import torch
    frame, desc = la.arrays(0)
    n, dim = desc.shape
    n0 = n - 700
    y = la.bearings_for(len(frame))
    xyz, cov = la.map_rows(n)
    with api.Landmarks(0) as L, api.Landmarks(0) as F:
        L.set(xyz[:n0], cov[:n0])
        L.set_descriptors(desc[:n0])
        L.append(xyz[n0:n0 + 300], cov[n0:n0 + 300])                     # a plain append: NaN rows
        got = L.get_descriptors()
        assert L.size == n0 + 300 and got[:n0].tobytes() == desc[:n0].tobytes() and np.isnan(got[n0:]).all()
        # the frame holds near copies of the undescribed rows' neighbours and of those rows themselves: none of them is associated
        ref = la.associate(frame, np.concatenate([desc[:n0], np.full((300, dim), np.nan, dtype=np.float32)]), 0.3)
        a = L.associate(frame, y, ratio=0.3)
        assert _bytes(a) == _want(ref, y) and (a.idx < n0).all() and la.expected(0, 0.3).idx.max() >= n0
        # described rows from the host, then from the device
        L.prune(mask=np.arange(L.size) < n0)
        L.append_described(xyz[n0:n0 + 300], cov[n0:n0 + 300], mc.strided(desc[n0:n0 + 300], "pad7_nan"))
        dev = torch.device("cuda:0")
        xd, cd, dd = (torch.from_numpy(np.array(a_)).to(dev) for a_ in (xyz[n0 + 300:], cov[n0 + 300:], desc[n0 + 300:]))
        torch.cuda.synchronize()
        L.append_described_device(xd.data_ptr(), cd.data_ptr(), dd.data_ptr(), n - n0 - 300, dim)
        assert L.size == n and L.get_descriptors().tobytes() == desc.tobytes()
        X, Cv = L.get()
        assert X.tobytes() == xyz.tobytes() and Cv.tobytes() == cov.tobytes()
        # ... which is a fresh handle's set + set_descriptors
        F.set(xyz, cov)
        all_d = torch.from_numpy(np.array(desc)).to(dev)
        torch.cuda.synchronize()
        F.set_descriptors_device(all_d.data_ptr(), n, dim)
        assert F.get_descriptors().tobytes() == desc.tobytes()
        assert _bytes(L.associate(frame, y)) == _bytes(F.associate(frame, y)) == _want(la.expected(0, 0.3), y)
        # refused: another dimension on a map that holds rows; allowed on an empty one, where it acts as set + set_descriptors
        with pytest.raises(cabi.SbaError):
            L.append_described(xyz[:2], cov[:2], np.zeros((2, dim + 1), dtype=np.float32))
        assert L.size == n and L.descriptor_dim == dim
        L.prune(mask=np.zeros(n, dtype=bool))
        L.append_described(xyz[:5], cov[:5], desc[:5, :7])
        assert L.size == 5 and L.descriptor_dim == 7 and L.get_descriptors().tobytes() == np.ascontiguousarray(desc[:5, :7]).tobytes()
        # set drops the descriptors
        L.set(xyz[:5], cov[:5])
        assert L.descriptor_dim == 0
        with pytest.raises(cabi.SbaError):
            L.associate(frame, y)


def test_an_undescribed_map_is_what_it_was():
    n = TILE + 5
    xyz, cov = la.map_rows(n, 3)
    mask = np.random.default_rng(81).random(n) < 0.5
    kept = np.flatnonzero(mask)
    with api.Landmarks(0) as L:
        L.set(xyz, cov)
        assert L.descriptor_dim == 0
        res = L.prune(mask=mask)
        assert np.array_equal(res.kept, kept)
        L.append(xyz[:7], cov[:7])
        want_x, want_c = np.concatenate([xyz[kept], xyz[:7]]), np.concatenate([cov[kept], cov[:7]])
        X, Cv = L.get()
        assert X.tobytes() == want_x.tobytes() and Cv.tobytes() == want_c.tobytes() and L.descriptor_dim == 0
        pick = np.array([3, 0, 3, len(want_x) - 1])
        gx, gc, gk = L.gather(pick)
        assert gx.tobytes() == want_x[pick].tobytes() and gc.tobytes() == want_c[pick].tobytes() and not gk.any()
        for call in (lambda: L.associate(np.zeros((4, 8), dtype=np.float32)), lambda: L.get_descriptors(),
                     lambda: L.append_described(xyz[:2], cov[:2], np.zeros((2, 8), dtype=np.float32))):
            with pytest.raises(cabi.SbaError) as e:
                call()
            assert e.value.code == cabi.SBA_ERR_INVALID_ARG
        assert L.size == len(want_x) and L.get()[0].tobytes() == want_x.tobytes()         # the handle stays usable


# ---- 4. histories, grids, runs ---------------------------------------------------------------------------------------------------------
def test_history_grid_and_run_independence(monkeypatch):
    k = 3
    frame, desc = la.arrays(k)
    n, dim = desc.shape
    y = la.bearings_for(len(frame))
    xyz, cov = la.map_rows(n)
    rng = np.random.default_rng(82)
    extra = mc._ints(rng, 900, dim) + 40.0                                # far from every frame row
    order = rng.permutation(n + 900)
    mixed_d = np.concatenate([desc, extra])[order]
    keep = order < n                                                     # the case's own rows, in a shuffled order
    want = None
    ref = la.associate(frame, mixed_d[keep], 0.3)
    assert ref.n_associated > 400
    for grid in (None, "1", "3"):
        if grid is None:
            monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
        else:
            monkeypatch.setenv("SBA_RESECT_GRID", grid)
        with api.Landmarks(0) as L, api.Landmarks(0) as F:
            mx, mcov = la.map_rows(n + 900, 5)
            L.set(mx, mcov)
            L.set_descriptors(mixed_d)
            L.prune(mask=keep)
            half = L.size // 2
            rows_d = mixed_d[keep]
            X, Cv = L.get()
            L.prune(mask=np.arange(L.size) < half)
            L.append_described(X[half:], Cv[half:], rows_d[half:])
            F.set(X, Cv)
            F.set_descriptors(rows_d)
            runs = [_bytes(H.associate(frame, y, ratio=0.3)) for H in (L, F, L)]
            assert runs[0] == runs[1] == runs[2] == _want(ref, y), grid
            assert L.get_descriptors().tobytes() == F.get_descriptors().tobytes() == rows_d.tobytes()
            want = runs[0] if want is None else want
            assert runs[0] == want, grid


# ---- 5. the chain: associate_device -> register_robust_device -------------------------------------------------------------------------
def test_associate_device_feeds_register_robust_device():
    import torch
    s = rb.solve_scene(513)
    n, dim = len(s.X), 64
    rng = np.random.default_rng(83)
    desc = mc._ints(rng, n, dim)
    seen = rng.permutation(n)[:400]                                      # a shuffled subset of the landmarks ...
    frame = np.concatenate([desc[seen], mc._ints(rng, 120, dim)])         # ... plus random rows
    for r in range(len(seen)):                                           # ... moved by +-1 in one or two entries
        cols = rng.choice(dim, size=rng.integers(1, 3), replace=False)
        frame[r, cols] += rng.choice([-1.0, 1.0], size=cols.size)
    stray = rng.normal(size=(120, 3))
    y = np.concatenate([s.y[seen], stray / np.linalg.norm(stray, axis=1, keepdims=True)])
    shuffle = rng.permutation(len(frame))
    frame, y = np.ascontiguousarray(frame[shuffle]), np.ascontiguousarray(y[shuffle])
    ref = la.associate(frame, desc, 0.3)
    assert ref.n_associated > 300 and set(ref.idx.tolist()) <= set(seen.tolist())
    kw = dict(huber_delta=rb.DELTA, bearing_sigma=s.bearing_sigma)
    dev = torch.device("cuda:0")
    with api.Landmarks(0) as A, api.Landmarks(0) as B:
        for H in (A, B):
            H.set(s.X, s.cov)
            H.set_descriptors(desc)
        f_dev, y_dev = torch.from_numpy(frame).to(dev), torch.from_numpy(y).to(dev)
        out = torch.full((3 * min(n, len(frame)),), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        a = A.associate_device(f_dev.data_ptr(), len(frame), dim, y_dev.data_ptr(), out.data_ptr(), ratio=0.3)
        assert _bytes(a) == _want(ref)
        got = A.register_robust(None, s.rot0, s.tran0, idx=a.idx, bearings_device=out.data_ptr(), options=api.default_lm_options(**TIGHT), **kw)
        host = B.register_robust(y[ref.rows], s.rot0, s.tran0, idx=ref.idx, options=api.default_lm_options(**TIGHT), **kw)
        for f in ("rot", "tran", "cov"):
            assert np.asarray(getattr(got, f)).tobytes() == np.asarray(getattr(host, f)).tobytes(), f
        counts = lambda f: (f.n_obs, f.n_skipped, f.n_behind, f.n_gated, f.n_fused, f.n_used, f.n_outlier)
        assert counts(got) == counts(host) and got.n_obs == ref.n_associated and got.n_fused > 0
        assert _state(A) == _state(B)
        assert A.get_descriptors().tobytes() == B.get_descriptors().tobytes() == desc.tobytes()      # register* leaves the descriptors alone
