"""GPU: the batched structure (Batch.structure_joint / structure_joint_into / structure_order_stats / structure_keep_below;
kernel csrc/sba_batch_structure.hip).

The batch of tests/test_gpu_batch_covariance.py: ten pairs of 0 ... 4097 matches whose row offsets 0, 0, 1, 4, 9, 72, 136, 201,
458, 971 put the pairs of 3, 63, 257 and 4097 matches on odd rows (the shifted 16-byte stores of xyz, the split store of the
score) and give every odd-sized pair a ragged last lane; 4097 is eight strides of a block and one match more and crosses the
tiles of the interleaved layout.  References: G Sigma G^T on the DENSE inverse (tests/structure_reference.py) up to 513 matches,
the long-double Schur form of tests/test_gpu_structure.py at 4097; then Problem.structure_joint on every pair alone, a batch of
one, the other pair layout, the lock-step driver and other blocks per pair.

Bounds: those of tests/test_gpu_structure.py, through structure_reference.check_structure --
    |X_i - ref|_max          <= TOL * |X_i|
    |Sigma_X,i - ref_i|_max  <= (2 kappa_i + kappa) * TOL * |ref_i|_max      and the same for q_i
with TOL = REL_TOL_F64 / REL_TOL_F32 and the scene conditions of cov_reference.kappa_limit asserted from the reference."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import ref_joint_numpy as rj
from cov_reference import kappa_limit, sin2_parallax
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api
from structure_reference import DenseStructure, check_structure, dense_structure
from test_gpu_batch_covariance import (DIM, GAUGES, LAYOUTS, OFFSETS, PLANTED, POINTS, SIZES, STORES, TOL, _cat, _fails, _opt,
                                       _planes, _same, _scene, _scenes, both, stores)
from test_gpu_structure import INF_ROW, schur_structure

pytestmark = pytest.mark.gpu

FIELDS = ("xyz", "cov", "score")


@lru_cache(maxsize=None)
def _refs(n, store, point):
    """{tran_param: reference} of the pair of size n, computed once and left unchanged."""
    c = _scene(n)
    x1, x2 = _planes(c.x1, c.x2, store)
    rot, tran = (c.rot_init, c.tran_init) if point == "init" else (c.rot_true, c.tran_true)
    if n > 513:
        return schur_structure(x1, x2, rot, tran, c.d12)
    return {tp: dense_structure(x1, x2, rot, tran, c.d12, tp) for tp in GAUGES if not _fails(n, tp)}


def _upload(b, store, cs=None):
    off, x1, x2, d12, rot, tran = _cat(cs or _scenes())
    b.upload(x1, x2, off, d12, store=store)
    return off, rot, tran


def _same_rows(a, b, what=""):
    """Two BatchJointStructure: the pose record and the three outputs, byte for byte."""
    _same(a.pose, b.pose, what)
    for k in FIELDS:
        assert (getattr(a, k) is None) == (getattr(b, k) is None), (what, k)
        if getattr(a, k) is not None:
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), (what, k)


def _assert_failed(r, g, lo, hi, tran_param=api.TRAN_SPHERE):
    assert r.status[g] == cabi.SBA_ERR_NUMERIC, g
    assert np.isnan(r.pose.cov[g]).all(), g
    for k in FIELDS:
        if getattr(r, k) is not None:
            assert np.isnan(getattr(r, k)[lo:hi]).all(), (g, k)
    assert r.dim[g] == DIM[tran_param] and r.dof[g] == r.n_used[g] - r.dim[g]


def test_the_batch_has_the_offsets_the_store_paths_need():
    """Every store path has a pair: first row even or odd (xyz: aligned or shifted 16-byte stores; score: one 16-byte store or
    two 8-byte stores), last lane whole or ragged (the padding match is never stored)."""
    off = _cat(_scenes())[0]
    assert tuple(int(v) for v in off) == OFFSETS
    paths = {(o % 2, n % 2) for n, o in zip(SIZES, OFFSETS) if n > 0}
    assert paths >= {(0, 0), (0, 1), (1, 1)}                     # 64 | 5, 65, 513 | 3, 63, 257, 4097 (whose inner lanes are (1, 0))
    assert [n for n, o in zip(SIZES, OFFSETS) if o % 2 == 1 and n > 0] == [3, 63, 257, 4097]
    assert sum(n % 2 for n in SIZES) == 8 and 4097 == 8 * 512 + 1
    assert (4097 + 1) // 2 > 256 * 3                             # three blocks per pair all have vectors to run


# ---- 1. the references, 2. the pose record ------------------------------------------------------------------------------------
@both
@stores
def test_against_the_references(monkeypatch, store, layout):
    """Largest err / bound: see the printed line (DESIGN.md section 3.16 records it)."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    worst = 0.0
    with api.Batch(0) as b:
        off, _, _ = _upload(b, store, cs)
        for point in POINTS:
            _, _, _, _, rot, tran = _cat(cs, point)
            for tran_param in GAUGES:
                with pytest.raises(api.SbaError) as ei:          # pairs of 0, 1 and 3 matches have no covariance
                    b.structure_joint(rot, tran, options=_opt(tran_param), xyz=False, cov=False)
                assert ei.value.code == cabi.SBA_ERR_NUMERIC
                r = b.structure_joint(rot, tran, options=_opt(tran_param), check=False)
                total = int(off[-1])
                assert r.xyz.shape == (total, 3) and r.cov.shape == (total, 6) and r.score.shape == (total,)
                assert np.array_equal(r.offsets, off.astype(np.int64))
                # 2. the pose record is covariance_joint's, byte for byte, status included
                _same(r.pose, b.covariance_joint(rot, tran, options=_opt(tran_param), depths=False, check=False), "pose")
                compared = 0
                for g, n in enumerate(SIZES):                    # every pair shown to the GPU is compared or asserted to have failed
                    lo, hi = int(off[g]), int(off[g + 1])
                    assert (r.n_used[g], r.n_degenerate[g]) == (n, 0), (g, n)
                    if _fails(n, tran_param):
                        _assert_failed(r, g, lo, hi, tran_param)
                        compared += 1
                        continue
                    ref = _refs(n, store, point)[tran_param]
                    assert ref.pose.kappa <= kappa_limit(n, tran_param), (n, ref.pose.kappa)
                    assert r.status[g] == 0 and (r.dim[g], r.dof[g]) == (ref.pose.m, n - ref.pose.m)
                    worst = max(worst, *check_structure(r.xyz[lo:hi], r.cov[lo:hi], r.score[lo:hi], ref, TOL[store],
                                                        what=f"batch n={n} store={store} layout={layout} gauge={tran_param} {point}"))
                    pg = r.pair(g)
                    assert all(getattr(pg, k).tobytes() == getattr(r, k)[lo:hi].tobytes() for k in FIELDS)
                    assert pg.pose.cov.tobytes() == r.pose.cov[g].tobytes() and pg.n_used == n
                    compared += 1
                assert compared == len(SIZES)
        # the default options are the sphere gauge
        d = b.structure_joint(rot, tran, check=False)
        assert (d.dim == 5).all()
        _same_rows(d, b.structure_joint(rot, tran, options=_opt(api.TRAN_SPHERE), check=False))
    print(f"largest err / bound store={store} layout={layout}: {worst:.3g}")


# ---- 3. bit-equalities --------------------------------------------------------------------------------------------------------
@stores
def test_layouts_drivers_blocks_per_pair_subsets_and_repeats_agree_bitwise(monkeypatch, store):
    cs = _scenes()
    got = {}
    for layout in LAYOUTS:
        monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
        with api.Batch(0) as b:
            off, rot, tran = _upload(b, store, cs)
            a = got[layout] = b.structure_joint(rot, tran, check=False)
            _same_rows(a, b.structure_joint(rot, tran, check=False), "two calls in a row")
            for bpp in ("1", "3"):
                monkeypatch.setenv("SBA_BATCH_STRUCTURE_BPP", bpp)
                got[layout, "bpp", bpp] = b.structure_joint(rot, tran, check=False)
            monkeypatch.delenv("SBA_BATCH_STRUCTURE_BPP")
            monkeypatch.setenv("SBA_BATCH_DEVICE_COV", "0")
            got[layout, "lock-step"] = b.structure_joint(rot, tran, check=False)
            monkeypatch.delenv("SBA_BATCH_DEVICE_COV")
            for want in range(8):                                   # every subset of the outputs against the all-outputs call
                kw = dict(xyz=bool(want & 1), cov=bool(want & 2), score=bool(want & 4))
                s = b.structure_joint(rot, tran, check=False, **kw)
                _same(a.pose, s.pose, ("subset", want))
                for k in FIELDS:
                    assert (getattr(s, k) is None) == (not kw[k])
                    if kw[k]:
                        assert getattr(s, k).tobytes() == getattr(a, k).tobytes(), (layout, want, k)
        _same_rows(a, got[layout, "bpp", "1"], "one block per pair")
        _same_rows(a, got[layout, "bpp", "3"], "three blocks per pair")
        _same_rows(a, got[layout, "lock-step"], "SBA_BATCH_DEVICE_COV=0")
    _same_rows(got["0"], got["1"], "layouts")
    valid = [g for g, n in enumerate(SIZES) if not _fails(n, api.TRAN_SPHERE)]
    for g in valid:
        lo, hi = int(off[g]), int(off[g + 1])
        assert all(np.isfinite(getattr(got["0"], k)[lo:hi]).all() for k in FIELDS) and (got["0"].score[lo:hi] > 0).all()


@stores
def test_a_pair_does_not_depend_on_its_batch(store):
    """Each pair alone in a batch of one (first row 0: even) against its rows in the full batch: the row parity differs for the
    pairs of 3, 63, 257 and 4097 matches, the values must not."""
    cs = _scenes()
    with api.Batch(0) as b:
        off, rot, tran = _upload(b, store, cs)
        r = b.structure_joint(rot, tran, check=False)
    for g, (n, c) in enumerate(zip(SIZES, cs)):
        lo, hi = int(off[g]), int(off[g + 1])
        with api.Batch(0) as b:
            b.upload(c.x1, c.x2, np.array([0, n], dtype=np.uint64), c.d12, store=store)
            a = b.structure_joint(c.rot_init[None], c.tran_init[None], check=False)
        assert a.status[0] == r.status[g], n
        assert a.pose.cov[0].tobytes() == r.pose.cov[g].tobytes(), n
        for k in FIELDS:
            assert getattr(a, k).tobytes() == getattr(r, k)[lo:hi].tobytes(), (n, k)


# ---- 4. the single problem ----------------------------------------------------------------------------------------------------
@both
@stores
def test_against_the_single_problem(monkeypatch, store, layout):
    """|batch - Problem.structure_joint| per pair within check_structure's bound: the two differ in the summation order of
    Sigma_c and in device-built pass parameters only.  The largest fraction of the bound is printed, not asserted."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    with api.Batch(0) as b:
        off, rot, tran = _upload(b, store, cs)
        got = {tp: b.structure_joint(rot, tran, options=_opt(tp), check=False) for tp in GAUGES}
    worst = 0.0
    for g, (n, c) in enumerate(zip(SIZES, cs)):
        lo, hi = int(off[g]), int(off[g + 1])
        with api.Problem(0) as p:
            if n > 0:
                p.upload(c.x1, c.x2, c.d12, store=store)
            for tp in GAUGES:
                r = got[tp]
                if _fails(n, tp):                                   # failing pairs fail on both sides
                    assert r.status[g] == cabi.SBA_ERR_NUMERIC
                    if n > 0:
                        with pytest.raises(api.SbaError) as ei:
                            p.structure_joint(c.rot_init, c.tran_init, options=_opt(tp))
                        assert ei.value.code == cabi.SBA_ERR_NUMERIC
                    continue
                one = p.structure_joint(c.rot_init, c.tran_init, options=_opt(tp))
                assert (r.n_used[g], r.n_degenerate[g], r.dim[g], r.dof[g]) == (one.n_used, one.n_degenerate, one.dim, one.dof)
                ref = DenseStructure()
                ref.xyz, ref.cov, ref.score, ref.pose = one.xyz, one.cov, one.score, _refs(n, store, "init")[tp].pose
                worst = max(worst, *check_structure(r.xyz[lo:hi], r.cov[lo:hi], r.score[lo:hi], ref, TOL[store],
                                                    what=f"single n={n} store={store} layout={layout} gauge={tp}"))
    print(f"largest |batch - single| / bound store={store} layout={layout}: {worst:.3g}")


# ---- 5. stores and guards -----------------------------------------------------------------------------------------------------
def _raw(b, name, rot, tran, *rest):
    lib = cabi.load_library()
    r_, t_ = np.ascontiguousarray(rot, dtype=np.float64), np.ascontiguousarray(tran, dtype=np.float64)
    return getattr(lib, name)(b._h, r_.ctypes.data_as(cabi._dp), t_.ctypes.data_as(cabi._dp), None, 0.0, *rest)


@stores
def test_host_form_writes_the_batchs_rows_and_nothing_else(store):
    """A batch uploaded with offsets[0] = 3: the raw C call on sentinel-filled arrays with 7 rows behind."""
    cs = _scenes()
    off, x1, x2, d12, rot, tran = _cat(cs)
    pad = lambda a: np.concatenate([np.zeros((3,) + a.shape[1:]), a])
    off3 = off + np.uint64(3)
    total = int(off3[-1])
    with api.Batch(0) as b:
        b.upload(pad(x1), pad(x2), off3, pad(d12), store=store)
        py = b.structure_joint(rot, tran, check=False)
        assert py.xyz.shape == (total, 3) and (py.xyz[:3] == 0).all() and (py.cov[:3] == 0).all() and (py.score[:3] == 0).all()
        out = (cabi.JointCov * len(cs))()
        X, Cv, q = np.full((total + 7, 3), -7.0), np.full((total + 7, 6), -7.0), np.full(total + 7, -7.0)
        st = np.full(len(cs), -99, dtype=np.int32)
        rc = _raw(b, "sba_batch_structure_joint", rot, tran, out, X.ctypes.data_as(cabi._dp), Cv.ctypes.data_as(cabi._dp),
                  q.ctypes.data_as(cabi._dp), st.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == cabi.SBA_ERR_NUMERIC and list(st) == list(py.status)
        for got, want in ((X, py.xyz), (Cv, py.cov), (q, py.score)):
            assert (got[:3] == -7.0).all() and (got[total:] == -7.0).all()
            assert not (got[3:total] == -7.0).any()                 # every row in between is written by exactly one pair
            assert got[3:total].tobytes() == want[3:].tobytes()
    # the shifted batch computes what the unshifted one does: only the row numbers differ (and their parity)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12, store=store)
        un = b.structure_joint(rot, tran, check=False)
    assert (un.xyz.tobytes(), un.cov.tobytes(), un.score.tobytes()) == (py.xyz[3:].tobytes(), py.cov[3:].tobytes(), py.score[3:].tobytes())


@stores
def test_device_form(store):
    cs = _scenes()
    dev = torch.device("cuda", 0)
    with api.Batch(0) as b:
        off, rot, tran = _upload(b, store, cs)
        total = int(off[-1])
        a = b.structure_joint(rot, tran, check=False)
        tx = torch.full((total + 2, 3), -7.0, dtype=torch.float64, device=dev)
        tc = torch.full((total + 2, 6), -7.0, dtype=torch.float64, device=dev)
        ts = torch.full((total + 2,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        with pytest.raises(api.SbaError) as ei:
            b.structure_joint_into(tx.data_ptr(), tc.data_ptr(), ts.data_ptr(), rot, tran)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
        tx.fill_(-7.0), tc.fill_(-7.0), ts.fill_(-7.0)
        torch.cuda.synchronize()
        pose = b.structure_joint_into(tx.data_ptr(), tc.data_ptr(), ts.data_ptr(), rot, tran, check=False)
        _same(a.pose, pose, "device form")
        hx, hc, hs = tx.cpu().numpy(), tc.cpu().numpy(), ts.cpu().numpy()
        assert (hx[:total].tobytes(), hc[:total].tobytes(), hs[:total].tobytes()) == (a.xyz.tobytes(), a.cov.tobytes(), a.score.tobytes())
        assert (hx[total:] == -7.0).all() and (hc[total:] == -7.0).all() and (hs[total:] == -7.0).all()
        # score only, NULL xyz / cov
        ts2 = torch.full((total + 2,), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        _same(a.pose, b.structure_joint_into(None, None, ts2.data_ptr(), rot, tran, check=False), "score only")
        h2 = ts2.cpu().numpy()
        assert h2[:total].tobytes() == a.score.tobytes() and (h2[total:] == -7.0).all()
        # a destination off by 8 bytes is refused and nothing is written
        for k in range(3):
            ptrs = [tx.data_ptr(), tc.data_ptr(), ts.data_ptr()]
            ptrs[k] += 8
            with pytest.raises(api.SbaError) as ei:
                b.structure_joint_into(*ptrs, rot, tran, check=False)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        assert (tx.cpu().numpy().tobytes(), tc.cpu().numpy().tobytes(), ts.cpu().numpy().tobytes()) == (hx.tobytes(), hc.tobytes(), hs.tobytes())


# ---- 6. degeneracy ------------------------------------------------------------------------------------------------------------
def _planted_batch(cs, point, store):
    """The batch with the matches of PLANTED made parallel at the pair's rot in what the planes hold; keep: the others."""
    off, x1, x2, d12, rot, tran = _cat(cs, point)
    x1, x2 = x1.copy(), x2.copy()
    keep = np.ones(len(x1), dtype=bool)
    for g, n in enumerate(SIZES):
        if n in PLANTED:
            rows = int(off[g]) + np.array(PLANTED[n])
            if store == api.STORE_F32:
                x1[rows] = x1[rows].astype(np.float32)
            x2[rows] = x1[rows] @ rj.rotation(rot[g]).T
            keep[rows] = False
    return off, x1, x2, d12, rot, tran, keep


@both
@stores
def test_degenerate_matches_are_left_out(monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    for point in POINTS:
        off, x1, x2, d12, rot, tran, keep = _planted_batch(cs, point, store)
        p1, p2 = _planes(x1, x2, store)
        with api.Batch(0) as b:
            b.upload(x1, x2, off, d12, store=store)
            r = b.structure_joint(rot, tran, min_sin2_parallax=1e-9, check=False)
        for g, n in enumerate(SIZES):
            lo, hi = int(off[g]), int(off[g + 1])
            if n not in PLANTED:
                assert r.n_degenerate[g] == 0 and r.n_used[g] == n
                assert (r.status[g] != 0) == _fails(n, api.TRAN_SPHERE)
                continue
            planted, kp = np.array(PLANTED[n]), keep[lo:hi]
            sin2 = sin2_parallax(p1[lo:hi], p2[lo:hi], rot[g])
            assert (sin2[planted] < 1e-10).all()
            assert not ((sin2[kp] >= 1e-10) & (sin2[kp] <= 1e-8)).any() and (sin2[kp] > 1e-8).all()
            ref = dense_structure(p1[lo:hi], p2[lo:hi], rot[g], tran[g], d12[lo:hi], api.TRAN_SPHERE, keep=kp)
            assert ref.pose.kappa <= kappa_limit(n, api.TRAN_SPHERE)
            assert r.status[g] == 0
            assert (r.n_degenerate[g], r.n_used[g], r.dof[g]) == (len(planted), n - len(planted), n - len(planted) - 5)
            xyz, cov, score = r.xyz[lo:hi], r.cov[lo:hi], r.score[lo:hi]
            assert np.array_equal(cov[planted], np.tile(INF_ROW, (len(planted), 1)))
            assert np.array_equal(score[planted], np.full(len(planted), np.inf))
            assert np.isfinite(xyz).all()
            assert np.abs(xyz[planted] - ref.xyz[planted]).max() <= TOL[store] * np.abs(ref.xyz[planted]).max()
            check_structure(xyz, cov, score, ref, TOL[store], used=np.flatnonzero(kp),
                            what=f"planted n={n} store={store} layout={layout} {point}")


# ---- 7. the cut ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def pinned_grid(monkeypatch):
    """Same grids for every handle (read at creation / upload): a compacted and a fresh batch reduce in the same order
    (tests/test_gpu_batch_quantile.py)."""
    monkeypatch.setenv("SBA_BLOCKS_PER_CU", "2")


@both
@stores
def test_the_cut(pinned_grid, monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    B = len(SIZES)
    off, x1, x2, d12, rot, tran, keep_planted = _planted_batch(cs, "init", store)
    kw = dict(min_sin2_parallax=1e-9)
    failed = np.array([_fails(n, api.TRAN_SPHERE) for n in SIZES])
    with api.Batch(0) as b, api.Batch(0) as fresh, api.Batch(0) as top:
        b.upload(x1, x2, off, d12, store=store)
        full = b.structure_joint(rot, tran, check=False, **kw)
        score = full.score
        assert np.array_equal(full.status != 0, failed)
        # order statistics: per pair elements of that pair's score rows, bit for bit; +inf on top; NaN for empty and failed pairs
        probs = (0.0, 0.25, 0.5, 1.0)
        ranks = b._pair_ranks(probs)
        with pytest.raises(api.SbaError) as ei:
            b.structure_order_stats(rot, tran, ranks, **kw)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
        vals, st = b.structure_order_stats(rot, tran, ranks, check=False, **kw)
        assert np.array_equal(st, full.status) and vals.shape == (B, len(probs))
        for g, n in enumerate(SIZES):
            lo, hi = int(off[g]), int(off[g + 1])
            if failed[g]:
                assert np.isnan(vals[g]).all(), n
                continue
            want = np.partition(score[lo:hi], ranks[g])[ranks[g]]
            assert vals[g].view(np.uint64).tolist() == want.view(np.uint64).tolist(), n
            assert (vals[g, -1] == np.inf) == (n in PLANTED)
        # keep_below: per pair exactly score <= 4 * q_(k), in order; failed pairs are intact
        with pytest.raises(api.SbaError) as ei:
            b.structure_keep_below(rot, tran, 0.5, 4.0, **kw)
        assert ei.value.code == cabi.SBA_ERR_NUMERIC
        assert len(b.offsets) == B + 1 and int(b.offsets[-1]) < int(off[-1])    # ... after the other pairs were cut: the wrapper follows
        b.upload(x1, x2, off, d12, store=store)                     # start again for the form that returns the result
        idx, noff, thr, st = b.structure_keep_below(rot, tran, 0.5, 4.0, check=False, **kw)
        assert np.array_equal(st, full.status) and idx.dtype == np.int64
        keep = np.zeros(len(score), dtype=bool)
        for g, n in enumerate(SIZES):
            lo, hi = int(off[g]), int(off[g + 1])
            if failed[g]:
                assert np.isnan(thr[g]), n
                keep[lo:hi] = True
                continue
            k = int(api.quantile_rank(0.5, n)[0])
            assert thr[g] == np.float64(4.0) * np.partition(score[lo:hi], k)[k], n
            keep[lo:hi] = score[lo:hi] <= thr[g]
            assert keep[lo:hi].sum() >= k + 1
        assert np.array_equal(idx, np.flatnonzero(keep)) and not keep[~keep_planted].any()
        assert np.array_equal(np.diff(noff.astype(np.int64)), [keep[int(off[g]):int(off[g + 1])].sum() for g in range(B)])
        assert np.array_equal(b.offsets, noff)
        # afterwards the batch equals a fresh upload of the kept rows
        fresh.upload(x1[idx], x2[idx], noff, d12[idx], store=store)
        assert b.blocks_per_pair == fresh.blocks_per_pair
        for mode in (api.MODE_ROT, api.MODE_TRAN, api.MODE_RT):
            for dm in (api.DEPTH_UNIFORM, api.DEPTH_PER_MATCH):
                f = lambda h: h.eval(mode, rot, tran, huber_delta=1.0, depth_mode=dm)
                assert f(b).tobytes() == f(fresh).tobytes(), (mode, dm)
        u, v = b.structure_joint(rot, tran, check=False, **kw), fresh.structure_joint(rot, tran, check=False, **kw)
        _same_rows(u, v, "kept rows")
        assert (u.n_degenerate == 0).all()
        # a rank on a +inf score: the threshold is +inf and every row of that pair stays
        top.upload(x1, x2, off, d12, store=store)
        idx, noff, thr, st = top.structure_keep_below(rot, tran, 1.0, 4.0, check=False, **kw)
        for g, n in enumerate(SIZES):
            if n in PLANTED:
                assert thr[g] == np.inf and int(noff[g + 1]) - int(noff[g]) == n
            elif not failed[g]:
                assert np.isfinite(thr[g])
            else:
                assert np.isnan(thr[g]) and int(noff[g + 1]) - int(noff[g]) == n


# ---- 8. state -----------------------------------------------------------------------------------------------------------------
def _counts(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_evaluations, s.initial_cost, s.final_cost, s.final_radius)


@both
@stores
def test_the_batch_is_left_alone(monkeypatch, store, layout):
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    cs = _scenes()
    off, x1, x2, d12, rot, tran = _cat(cs)
    dev = torch.device("cuda", 0)
    with api.Batch(0) as b, api.Batch(0) as twin:
        b.upload(x1, x2, off, d12, store=store)
        twin.upload(x1, x2, off, d12, store=store)
        b.structure_joint(rot, tran, check=False)
        ts = torch.empty(int(off[-1]), dtype=torch.float64, device=dev)
        b.structure_joint_into(None, None, ts.data_ptr(), rot, tran, check=False)
        b.structure_order_stats(rot, tran, b._pair_ranks([0.5]), check=False)
        # solve_joint after the structure calls == solve_joint on a twin without them
        u, v = b.solve_joint(rot, tran, check=False), twin.solve_joint(rot, tran, check=False)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(u[:3], v[:3])) and u[4].tobytes() == v[4].tobytes()
        assert [_counts(s) for s in u[3]] == [_counts(s) for s in v[3]]
        # ... and so is the d-only stage
        b.structure_joint(u[0], u[1], check=False)
        du, dv = b.solve_depths(u[0], u[1]), twin.solve_depths(v[0], v[1])
        assert du[0].tobytes() == dv[0].tobytes() and du[2].tobytes() == dv[2].tobytes()
    # after keep_below the structure is that of a fresh upload of the kept rows
    with api.Batch(0) as b, api.Batch(0) as fresh:
        b.upload(x1, x2, off, d12, store=store)
        b.structure_joint(rot, tran, check=False)
        idx, noff, _ = b.keep_below(rot, tran, 0.9, 1.0, depth_mode=api.DEPTH_PER_MATCH)
        assert 0 < len(idx) < len(x1)
        fresh.upload(x1[idx], x2[idx], noff, d12[idx], store=store)
        _same_rows(b.structure_joint(rot, tran, check=False), fresh.structure_joint(rot, tran, check=False), "kept rows")


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def _entry_points(b, rot, tran, **kw):
    return {
        "structure_joint": lambda: b.structure_joint(rot, tran, **kw),
        "structure_joint_into": lambda: b.structure_joint_into(None, None, None, rot, tran, **kw),
        "structure_order_stats": lambda: b.structure_order_stats(rot, tran, [0], **kw),
        "structure_keep_below": lambda: b.structure_keep_below(rot, tran, 0.5, 4.0, **kw),
    }


def _refused(b, rot, tran, code, **kw):
    for name, f in _entry_points(b, rot, tran, **kw).items():
        with pytest.raises(api.SbaError) as ei:
            f()
        assert ei.value.code == code, name


def test_refusals(monkeypatch):
    cs = _scenes()
    off, x1, x2, d12, rot, tran = _cat(cs)
    B = len(cs)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    with api.Batch(0) as b:
        z = np.zeros((0, 3))
        _refused(b, z, z, cabi.SBA_ERR_NOT_UPLOADED)
        out10 = (cabi.JointCov * B)()
        for name in ("sba_batch_structure_joint", "sba_batch_structure_joint_device"):
            assert _raw(b, name, rot, tran, out10, None, None, None, None) == cabi.SBA_ERR_NOT_UPLOADED
        b.upload(x1, x2, off)                             # uniform depths: no per-match planes
        _refused(b, rot, tran, cabi.SBA_ERR_UNSUPPORTED)
        b.upload(x1, x2, off, d12)
        before = b.structure_joint(rot, tran, check=False)
        valid = np.array([not _fails(n, api.TRAN_SPHERE) for n in SIZES])
        assert np.array_equal(before.status == 0, valid)
        for bad in (-1.0, float("nan")):
            _refused(b, rot, tran, cabi.SBA_ERR_INVALID_ARG, min_sin2_parallax=bad)
        for name in ("sba_batch_structure_joint", "sba_batch_structure_joint_device"):
            assert _raw(b, name, rot, tran, None, None, None, None, None) == cabi.SBA_ERR_INVALID_ARG           # a NULL out
        # a rank that is not below its pair's size (pair of 5 matches); scales that are not finite or negative
        ranks = np.zeros((B, 1), dtype=np.uintp)
        ranks[SIZES.index(5), 0] = 5
        with pytest.raises(api.SbaError) as ei:
            b.structure_order_stats(rot, tran, ranks)
        assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        thr, nk, sc = np.zeros(B), np.zeros(B, dtype=np.uintp), np.full(B, 4.0)
        rk = np.ascontiguousarray(ranks[:, 0])
        sz = lambda a: a.ctypes.data_as(C.POINTER(C.c_size_t))
        assert _raw(b, "sba_batch_structure_keep_below", rot, tran, sz(rk), sc.ctypes.data_as(cabi._dp), thr.ctypes.data_as(cabi._dp),
                    sz(nk), None, None) == cabi.SBA_ERR_INVALID_ARG
        for scale in (-1.0, float("inf"), float("nan")):
            with pytest.raises(api.SbaError) as ei:
                b.structure_keep_below(rot, tran, 0.5, scale)
            assert ei.value.code == cabi.SBA_ERR_INVALID_ARG
        assert np.array_equal(b.offsets, off)
        # a pair with a non-finite rot fails alone, the other pairs keep their earlier bytes
        g_bad = SIZES.index(257)
        bad = rot.copy(); bad[g_bad, 1] = np.inf
        r = b.structure_joint(bad, tran, check=False)
        expect = valid.copy(); expect[g_bad] = False
        assert np.array_equal(r.status == 0, expect) and (r.status[~expect] == cabi.SBA_ERR_NUMERIC).all()
        _assert_failed(r, g_bad, int(off[g_bad]), int(off[g_bad + 1]))
        for g in np.flatnonzero(expect):
            lo, hi = int(off[g]), int(off[g + 1])
            assert r.pose.cov[g].tobytes() == before.pose.cov[g].tobytes()
            assert all(getattr(r, k)[lo:hi].tobytes() == getattr(before, k)[lo:hi].tobytes() for k in FIELDS)
        # every match degenerate: every pair fails, the call says so, nothing is cut, the handle works afterwards
        _refused(b, rot, tran, cabi.SBA_ERR_NUMERIC, min_sin2_parallax=2.0)
        assert np.array_equal(b.offsets, off)
        r = b.structure_joint(rot, tran, min_sin2_parallax=2.0, check=False)
        assert (r.status == cabi.SBA_ERR_NUMERIC).all() and all(np.isnan(getattr(r, k)).all() for k in FIELDS)
        assert (r.n_used == 0).all() and np.array_equal(r.n_degenerate, np.array(SIZES))
        idx, noff, thr, st = b.structure_keep_below(rot, tran, 0.5, 4.0, min_sin2_parallax=2.0, check=False)
        assert np.array_equal(idx, np.arange(int(off[-1]))) and np.array_equal(noff, off) and np.isnan(thr).all() and (st != 0).all()
        _same_rows(b.structure_joint(rot, tran, check=False), before, "after the failures")
    monkeypatch.setenv("SBA_PUBLISH", "0")
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12)
        _refused(b, rot, tran, cabi.SBA_ERR_UNSUPPORTED)
